"""The wire-path edge helper (tests/wire_edges.py) pinned to independent
references, and its byte-classification table run through the host cipher
(csrc/host_aes.cpp, AES-NI and table).  No GPU.

The unit arithmetic against dn_aes_encrypt_len / dn_aes_decrypt_capacity; the
numpy record builder against oracle/py_shamir.share_to_bytes, record by
record; the tile filler against field.limbs_to_vec; `canonical()` against the
reference's own parsers (bytes.fromhex, base64.b64decode) for every text the
GPU classification test builds.
"""
import base64
import ctypes
import random

import numpy as np
import pytest

import wire_edges as we
from delta_node.crypto.aes import aes as aes_mod
from delta_node.crypto.shamir import _native, field
from oracle.py_shamir import share_to_bytes
from test_host_aes import impl  # noqa: F401  (fixture: the AES-NI and the table host cipher)


def test_unit_arithmetic_equals_the_length_functions():
    L = aes_mod._lib()
    big = [we.n_for_units(we.two_pass_units(cus * we.GROUP), 5) for cus in (8, 256, 304)]
    totals = [t - 16 for t in we.EDGE_ENC_TOTALS]
    for n in list(range(401)) + we.CANON_SIZES + totals + big + [we.class_n(p) for p in we.CLASS_RAGGED]:
        for hex_ in (False, True):
            size = int(L.dn_aes_encrypt_len(n, int(hex_)))
            assert size == we.text_len(n, hex_), (n, hex_)
            assert int(L.dn_aes_decrypt_capacity(size, int(hex_))) == we.plain_capacity(size, hex_) == n + we.pad_chars(n)
        chars = int(L.dn_aes_encrypt_len(n, 0))
        assert we.enc_units(n) == we.text_units(n) == (chars + 63) // 64 == -(-(n + 16) // 48)
        assert base64.b64encode(bytes(n + 16)).count(b"=") == we.pad_chars(n)
    for n_text in range(401):
        for hex_ in (False, True):
            assert int(L.dn_aes_decrypt_capacity(n_text, int(hex_))) == we.plain_capacity(n_text, hex_)


def test_n_for_units_and_wave_predicates():
    for u in list(range(2, 140)) + [we.two_pass_units(256 * we.GROUP)]:
        for ragged in (1, 5, 47, 48):
            n = we.n_for_units(u, ragged)
            assert we.enc_units(n) == we.text_units(n) == u
            assert (n + 16) - 48 * (u - 1) == ragged
            assert we.enc_whole(n, u - 1) == (ragged == 48) and not we.enc_whole(n, 0)
            assert all(we.enc_whole(n, g) for g in (1, u - 2) if 1 <= g <= u - 2)
    # the shapes the GPU tests name: one unit short of a full wave, exactly full, full + 1
    assert [we.dec_wave_full(u, 0) for u in (65, 66, 67)] == [False, True, True]
    assert [we.dec_whole(u, 65) for u in (66, 67)] == [False, True]
    assert [we.dec2_wave_full(u, 1) for u in (128, 129, 130)] == [False, True, True]
    assert [we.enc_wave_full(t - 16, 1) for t in we.EDGE_ENC_TOTALS] == [False, True, True]
    assert [we.enc_units(t - 16) for t in we.EDGE_ENC_TOTALS] == [128, 128, 129]
    assert not we.enc_wave_full(6144 - 16, 0)  # unit 0 holds the nonce
    assert we.locate(1 + 3 * 4096 + 64 * 5 + 9, 4096, first_unit=1) == (1 + 3 * 4096 + 329, 3, 5, 9)
    assert int.from_bytes(we.nonce_wrapping_at(40), "big") + 40 == 1 << 128


def _edge_values():
    rng = random.Random(5)
    vals = [0] + [1 << (8 * b - 1) for b in range(1, 66)] + [(1 << (8 * b)) - 1 for b in range(1, 66)]
    vals += [1 << 520, we.P - 1, 1 << 512, (1 << 512) - 1]
    vals += [rng.randrange(we.P) >> rng.randrange(0, 521) for _ in range(300)]
    return vals


@pytest.mark.parametrize("x", [0, 1, 255, 256, 1 << 56, (1 << 64) - 1])
def test_record_builder_equals_share_to_bytes(x):
    vals = _edge_values()
    assert {(v.bit_length() + 7) // 8 for v in vals} == set(range(67))  # every byte length 0..66
    limbs = we.ints_to_limbs(vals)
    assert we.limbs_to_ints(limbs) == vals and np.array_equal(limbs, field.ints_to_limbs(vals))
    assert we.y_lengths(limbs).tolist() == [(v.bit_length() + 7) // 8 for v in vals]
    packed, offs = we.build_records(x, limbs)
    buf = packed.tobytes()
    for e, v in enumerate(vals):
        assert buf[offs[e]:offs[e + 1]] == share_to_bytes(x, v), (e, v)
    assert offs[0] == 0 and offs[-1] == len(buf)
    # the sparse form: the same values scattered over a longer, otherwise zero vector
    n = 7 * len(vals) + 3
    index = np.arange(len(vals), dtype=np.int64) * 7 + 2
    packed, offs = we.build_records(x, limbs, n=n, index=index)
    dense = [0] * n
    for i, v in zip(index.tolist(), vals):
        dense[i] = v
    assert packed.tobytes() == b"".join(share_to_bytes(x, v) for v in dense)
    assert offs.tolist() == np.cumsum([0] + [len(share_to_bytes(x, v)) for v in dense]).tolist()


def test_ragged_limbs_and_sparse_plan():
    limbs = we.ragged_limbs(70001, 3)
    vals = we.limbs_to_ints(limbs[:2000])
    assert all(v < we.P for v in vals)
    assert set(we.y_lengths(limbs).tolist()) == set(range(67))
    n = we.SCAN2_N
    assert n == 8192 * 1024 + 1025 and -(-n // we.SCAN_BLOCK) == 8194 > we.SCAN_STAGE
    index, nbytes, lim = we.sparse_values(n)
    assert np.array_equal(we.y_lengths(lim), nbytes) and index[-1] == n - 1
    assert (lim[nbytes == 66, 16] != 0).all() and (lim[nbytes == 64, 16] == 0).all()
    for j in we.SCAN2_EDGES:  # both sides of every edge, one 66 and one 64 bytes
        at = [int(nbytes[np.searchsorted(index, e)]) for e in (1024 * j - 1, 1024 * j)]
        assert sorted(at) == [64, 66], (j, at)
    small = index[nbytes <= 3]
    assert (small % we.SPARSE_STEP == 0).all() and set(nbytes[nbytes <= 3].tolist()) == {1, 2, 3}
    assert small.size >= n // we.SPARSE_STEP - 2 * len(we.SCAN2_EDGES) - 1
    assert all(v < we.P for v in we.limbs_to_ints(lim))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 70001])
def test_tile_fillers_equal_limbs_to_vec(n):
    limbs = we.ragged_limbs(n, n)
    want = field.limbs_to_vec(limbs)
    assert want.size == we.vec_bytes(n) == field.vec_bytes(n)
    assert np.array_equal(we.tiles_of(limbs), want)
    vec = np.full(we.vec_bytes(n), 0xEE, dtype=np.uint8)

    def put(off, b):
        vec[off:off + b.size] = b

    we.fill_tiles(put, limbs, chunk_tiles=3)
    assert np.array_equal(vec, want)
    index = np.arange(0, n, 7, dtype=np.int64)
    sparse = np.zeros_like(limbs)
    sparse[index] = limbs[index]
    vec = np.zeros(we.vec_bytes(n), dtype=np.uint8)
    pos, val = we.scatter_tiles(index, limbs[index])
    vec[pos] = val
    assert np.array_equal(vec, field.limbs_to_vec(sparse))


def _reference_accepts(text: bytes, hex_: bool) -> bool:
    """The reference's own parsers, strict: bytes.fromhex then
    b64decode(validate=True) accept the text, the result holds a nonce, and
    re-encoding gives back the same length (nothing was skipped)."""
    try:
        b64 = bytes.fromhex(text.decode("ascii")) if hex_ else text
        if hex_ and 2 * len(b64) != len(text):
            return False
        raw = base64.b64decode(b64, validate=True)
    except ValueError:  # binascii.Error and UnicodeDecodeError are ValueErrors
        return False
    return len(raw) >= 16 and len(base64.b64encode(raw)) == len(b64)


def test_canonical_agrees_with_the_reference_parsers():
    count = 0
    for label, hex_, text, positions in we.class_texts():
        assert we.canonical(text, hex_) and _reference_accepts(text, hex_)
        for pos in positions:
            for value in range(256):
                t = we.substitute(text, pos, value)
                assert we.canonical(t, hex_) == _reference_accepts(t, hex_), (label, pos, value)
                count += 1
    assert count >= 6000
    for t, hex_ in ((b"", False), (b"A" * 20, False), (b"A" * 25, False), (b"0x" + b"41" * 24, True), (b"41" * 24, True),
                    (b"414", True), (b"A" * 21 + b"===", False), (b"A" * 24 + b"====", False)):
        assert we.canonical(t, hex_) == _reference_accepts(t, hex_), t


def test_classification_table_on_the_host_cipher(impl):
    """dn_aes_decrypt_host returns DN_ERR_RETRY exactly for the texts that are
    not canonical, and the reference's plaintext for the others."""
    L = aes_mod._lib()
    key = we.CLASS_KEY
    for label, hex_, text, positions in we.class_texts():
        cap = we.plain_capacity(len(text), hex_)
        out, n = ctypes.create_string_buffer(cap), ctypes.c_uint64()
        for pos in positions:
            for value in range(256):
                t = we.substitute(text, pos, value)
                rc = L.dn_aes_decrypt_host(key, len(key), t, len(t), int(hex_), out, cap, ctypes.byref(n))
                if we.canonical(t, hex_):
                    assert rc == _native.DN_OK, (label, pos, value)
                    assert out.raw[: n.value] == we.ref_decrypt(key, t, hex_), (label, pos, value)
                else:
                    assert rc == _native.DN_ERR_RETRY, (label, pos, value)
