"""The envelope kernels (csrc/aes_envelope.hip) where test_gpu_aes.py's shapes
do not reach: the device's own answer for canonical text (decrypt_vec hides
it behind a host re-parse whenever the kernel flags the text), the
wave-fullness edges of the coalesced text paths at every input skew, the
second and third grid-stride pass of every kernel, every byte value at every
kind of text position, and guard bands around each output.

Expected values: oracle/aes_oracle.c through tests/wire_edges.py, Python's
base64 / bytes.fromhex; bit-exact.  Each test asserts the premise it needs
(a full wave, units beyond two strides) by wire_edges' arithmetic.
"""
import contextlib

import pytest
import torch

import wire_edges as we
from delta_node.crypto import aes
from delta_node.crypto.aes import aes as aes_mod
from delta_node.crypto.shamir import _native
from oracle import c_oracle
from test_gpu_aes import KEYS, NONCES, SIZES

pytestmark = pytest.mark.gpu

LAYOUTS = ["product", "two-table"]
CANARY = 0xA5


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@contextlib.contextmanager
def layout(name, monkeypatch):
    """The product library, or the tuning build's 64-KB two-table layout, whose
    decrypt is the two-pass decode_kernel + ctr_text_kernel (32-byte keys)."""
    if name == "product":
        yield
        return
    monkeypatch.setenv("DN_AES_TABLES", "2")
    with _native.library(_native.TUNING_LIB):
        yield


def host(t) -> bytes:
    return bytes(t.cpu().numpy())


def stage(b: bytes, skew: int = 0, fill: int = 0):
    """b on the device `skew` bytes into a fresh allocation that ends with the
    16-byte granule of b's last byte; every other byte of it is `fill`.  The
    kernels read whole granules, so whatever they take from the slack must not
    show in a result."""
    total = max(16, (skew + len(b) + 15) // 16 * 16)
    buf = torch.full((total,), fill, dtype=torch.uint8, device=dev())
    assert buf.data_ptr() % 16 == 0
    if b:
        buf[skew:skew + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev())
    return buf[skew:skew + len(b)]


def raw_decrypt(key, text, hex_, slack=0):
    """dn_aes_decrypt as decrypt_vec calls it, but the device's own answer:
    (rc, out, out_len, bad).  text: device tensor without "0x"; out has
    `slack` canary bytes of capacity beyond dn_aes_decrypt_capacity."""
    L = aes_mod._lib()
    n_text = text.numel()
    cap = int(L.dn_aes_decrypt_capacity(n_text, int(hex_)))
    out = torch.full((max(cap + slack, 16),), CANARY, dtype=torch.uint8, device=text.device)
    meta = torch.zeros(2, dtype=torch.int64, device=text.device)
    rc = L.dn_aes_decrypt(key, len(key), text.data_ptr(), n_text, int(hex_), out.data_ptr(), cap + slack,
                          meta.data_ptr(), meta.data_ptr() + 8, _native.stream_ptr())
    out_len, bad = meta.tolist()
    return rc, out, out_len, bad


def assert_opens(key, text, hex_, data: bytes, what):
    rc, out, out_len, bad = raw_decrypt(key, text, hex_)
    assert (rc, bad, out_len) == (0, 0, len(data)), what
    assert host(out[:len(data)]) == data, what


# ---------------------------------------------------------------- 1. canonical text stays on the device
@pytest.mark.parametrize("lib", LAYOUTS)
def test_canonical_text_is_decrypted_on_the_device(lib, monkeypatch):
    """decrypt_vec re-parses on the host whenever the kernel sets *bad, so a
    kernel that flagged canonical text would pass every decrypt_vec test: here
    the flag itself must stay 0 and the device's bytes are compared."""
    assert set(SIZES) | {6127} <= set(we.CANON_SIZES)
    units = {we.text_units(n) for n in we.CANON_SIZES}
    assert {65, 66, 67, 129, 130, 131} <= units
    assert we.dec_wave_full(66, 0) and not we.dec_wave_full(65, 0) and we.dec2_wave_full(129, 1)
    key, nonce = KEYS[0], NONCES[4]
    with layout(lib, monkeypatch):
        for n in we.CANON_SIZES:
            data = we.rand_bytes(n, 1000 + n)
            b64, hx = we.want_text(key, nonce, data), we.want_text(key, nonce, data, True)
            assert_opens(key, stage(b64), False, data, (n, "base64"))
            assert_opens(key, stage(hx), True, data, (n, "hex"))
            after_0x = stage(b"0x" + hx)[2:]
            assert after_0x.data_ptr() % 16 == 2
            assert_opens(key, after_0x, True, data, (n, "hex after 0x"))
            assert_opens(key, stage(hx.upper()), True, data, (n, "upper-case hex"))


# ---------------------------------------------------------------- 2. wave fullness x skew
@pytest.mark.parametrize("skew", we.SKEWS)
@pytest.mark.parametrize("lib", LAYOUTS)
def test_decrypt_wave_edges_at_every_skew(lib, skew, monkeypatch):
    """One unit short of a full wave, exactly one full wave before the ragged
    last unit (lane 63's last chunk is then that unit's line), and a full wave
    plus one whole unit — for the fused kernel (65-67 units) and the two-pass
    decode (129-131).  The slack of the text's allocation is filled with two
    patterns: the result depends on neither."""
    assert [we.dec_wave_full(u, 0) for u in (65, 66, 67)] == [False, True, True] and not we.dec_whole(66, 65)
    assert [we.dec2_wave_full(u, 1) for u in (128, 129, 130)] == [False, True, True] and not we.dec_whole(129, 128)
    key, nonce = KEYS[0], NONCES[2]
    with layout(lib, monkeypatch):
        for u in we.EDGE_DEC_UNITS:
            for ragged in (1, 20, 48):
                n = we.n_for_units(u, ragged)
                assert we.text_units(n) == u
                data = we.rand_bytes(n, 31 * u + ragged)
                for hex_ in (False, True):
                    text = we.want_text(key, nonce, data, hex_)
                    for fill in (0x41, 0xBD):  # a character of both alphabets, and one of neither
                        t = stage(text, skew, fill)
                        assert t.data_ptr() % 16 == skew
                        assert_opens(key, t, hex_, data, (u, ragged, hex_, hex(fill)))


@pytest.mark.parametrize("skew", we.SKEWS)
@pytest.mark.parametrize("lib", LAYOUTS)
def test_encrypt_and_ctr_wave_edges_at_every_skew(lib, skew, monkeypatch):
    """n + 16 = 48 * 128 - 1, 48 * 128, 48 * 128 + 1: the last wave of encrypt
    one byte short of whole units, whole (its last store a coalesced one), and
    whole with a ragged unit after it; the plaintext read at every skew from an
    allocation that ends with its last granule."""
    assert [we.enc_wave_full(t - 16, 1) for t in we.EDGE_ENC_TOTALS] == [False, True, True]
    key, nonce = KEYS[0], NONCES[2]
    with layout(lib, monkeypatch):
        for total in we.EDGE_ENC_TOTALS:
            n = total - 16
            data = we.rand_bytes(n, total)
            ct = c_oracle.aes_ctr(key, nonce, data)
            for fill in (0x00, 0xFF):
                d = stage(data, skew, fill)
                assert d.data_ptr() % 16 == skew
                assert host(aes.ctr_vec(key, nonce, d)) == ct, (total, hex(fill))
                for hex_ in (False, True):
                    want = (b"0x" if hex_ else b"") + we.want_text(key, nonce, data, hex_)
                    assert host(aes.encrypt_vec(key, d, nonce=nonce, hex=hex_)) == want, (total, hex_, hex(fill))


# ---------------------------------------------------------------- 3. second and third pass
def stride_units() -> int:
    """Units (16-byte blocks for ctr) one pass of a capped grid covers: one
    1024-thread workgroup per CU, or two of 512 in the two-table layout."""
    return torch.cuda.get_device_properties(dev()).multi_processor_count * we.GROUP


class Big:
    """One message beyond two strides of every envelope kernel, its oracle
    ciphertext and texts, on the host and on the device (computed once)."""

    def __init__(self, key, units, ragged, nonce):
        self.key, self.nonce, self.units = key, nonce, units
        self.n = we.n_for_units(units, ragged)
        self.data = we.rand_bytes(self.n, units % 1000)
        self.ct = c_oracle.aes_ctr(key, nonce, self.data)
        self.b64 = we.want_text(key, nonce, self.data)
        self.d_data, self.d_ct, self.d_b64 = (self.up(b) for b in (self.data, self.ct, self.b64))
        self._hex = None

    @staticmethod
    def up(b: bytes, skew: int = 0):
        buf = torch.empty(len(b) + skew + 16, dtype=torch.uint8, device=dev())
        assert buf.data_ptr() % 16 == 0
        buf[skew:skew + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev())
        return buf[skew:skew + len(b)]

    @property
    def d_hex(self):
        if self._hex is None:
            self._hex = self.up(self.b64.hex().encode())
        return self._hex


@pytest.fixture(scope="module")
def big256():
    S = stride_units()
    big = Big(KEYS[0], we.two_pass_units(S), 5, we.nonce_wrapping_at(3 * S + 40))
    yield big
    del big
    torch.cuda.empty_cache()


def assert_same(got, want, what, unit_bytes, stride, first_unit=0, shift=0):
    """Whole-message equality on the device; the first differing byte is
    reported as the (unit, pass, wave, lane) of the thread that wrote it."""
    assert got.numel() == want.numel(), (what, got.numel(), want.numel())
    if torch.equal(got, want):
        return
    i = int((got != want).nonzero()[0].item())
    where = we.locate((i + shift) // unit_bytes, stride, first_unit)
    pytest.fail(f"{what}: first difference at byte {i} of {want.numel()}: (unit, pass, wave, lane) = {where}, "
                f"got {int(got[i])} want {int(want[i])}")


def check_all(big: Big, skew: int, ops=("ctr", "enc64", "enchex", "dec64", "dechex"), fused=True):
    S = stride_units()
    key, nonce, n = big.key, big.nonce, big.n
    data = big.d_data if skew == 0 else Big.up(big.data, skew)
    assert data.data_ptr() % 16 == skew
    if "ctr" in ops:
        assert -(-n // 16) > 2 * S
        assert_same(aes.ctr_vec(key, nonce, data), big.d_ct, "ctr_vec", 16, S)
    if "enc64" in ops:
        assert_same(aes.encrypt_vec(key, data, nonce=nonce), big.d_b64, "encrypt_vec base64", 64, S)
    if "enchex" in ops:
        assert_same(aes.encrypt_vec(key, data, nonce=nonce, hex=True)[2:], big.d_hex, "encrypt_vec hex", 128, S)
    for op, hex_ in (("dec64", False), ("dechex", True)):
        if op not in ops:
            continue
        text = big.d_hex if hex_ else big.d_b64
        if skew:
            moved = torch.empty(text.numel() + skew + 16, dtype=torch.uint8, device=dev())
            moved[skew:skew + text.numel()] = text
            text = moved[skew:skew + text.numel()]
        assert text.data_ptr() % 16 == skew
        rc, out, out_len, bad = raw_decrypt(key, text, hex_)
        assert (rc, bad, out_len) == (0, 0, n), (op, rc, bad, out_len)
        # plaintext byte i belongs to unit (i + 16) // 48; the fused kernel's thread t takes unit 1 + t,
        # the two-pass decode_kernel's (256-thread workgroups, 8 per CU) unit t
        dstride, dfirst = (S, 1) if fused else (2 * S, 0)
        assert_same(out[:n], big.d_data, "dn_aes_decrypt " + ("hex" if hex_ else "base64"), 48, dstride, dfirst, shift=16)


@pytest.mark.slow
@pytest.mark.parametrize("skew", [0, 5])
@pytest.mark.parametrize("lib", LAYOUTS)
def test_second_and_third_pass_whole_message(lib, skew, big256, monkeypatch):
    """A capped grid's threads take a second unit only beyond CUs x 1024 units
    (two-pass decode: CUs x 2048): U = 2 S + 2 * 64 + 7 units run the next-unit
    prefetch of every kernel in a second pass with full waves and a ragged one;
    the 128-bit counter wraps inside a full wave of encrypt's second pass."""
    S = stride_units()
    U = big256.units
    assert U > 2 * S and we.text_units(big256.n) == we.enc_units(big256.n) == U
    assert we.enc_wave_full(big256.n, 2 * S // 64) and we.enc_wave_full(big256.n, 2 * S // 64 + 1)
    assert we.dec_wave_full(U, 2 * S // 64) and we.dec2_wave_full(U, 2 * S // 64 + 1) and not we.dec_whole(U, U - 1)
    wrap_unit = (3 * S + 40 + 1) // 3  # the unit holding keystream block 3 S + 40
    assert we.locate(wrap_unit, S)[1] == 1 and we.enc_wave_full(big256.n, wrap_unit // 64)
    assert int.from_bytes(big256.nonce, "big") + 3 * S + 40 == 1 << 128
    with layout(lib, monkeypatch):
        check_all(big256, skew, fused=lib == "product")


@pytest.mark.slow
@pytest.mark.parametrize("key", KEYS[1:], ids=["aes128", "aes192"])
def test_second_pass_other_key_sizes(key):
    S = stride_units()
    big = Big(key, S + 64 + 3, 5, we.nonce_wrapping_at(3 * S + 40))
    assert big.units > S and we.enc_wave_full(big.n, S // 64) and we.dec_wave_full(big.units, S // 64)
    check_all(big, 0, ops=("ctr", "enc64", "dec64"))
    del big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 4. byte classification
@pytest.mark.parametrize("case", range(4), ids=["base64==", "base64=", "base64", "hex"])
def test_every_byte_value_at_every_kind_of_position(case):
    """bad != 0 exactly when the text is not canonical, for all 256 values at a
    digit / character of each lane of a word in a coalesced wave and in a unit
    read per lane, in the nonce, in the last unit and in the padding; when the
    kernel accepts, its plaintext is the reference's.  Then decrypt_vec on a
    sample of the flagged texts does what the reference does."""
    label, hex_, text, positions = we.class_texts()[case]
    key = we.CLASS_KEY
    base = stage(text)
    flagged = []
    for pos in positions:
        for value in range(256):
            t = base.clone()
            t[pos] = value
            sub = we.substitute(text, pos, value)
            rc, out, out_len, bad = raw_decrypt(key, t, hex_)
            assert rc == 0, (label, pos, value)
            if not we.canonical(sub, hex_):
                assert bad != 0, (label, pos, value, "not flagged")
                flagged.append((pos, value))
                continue
            assert bad == 0, (label, pos, value, "canonical text flagged")
            assert host(out[:out_len]) == we.ref_decrypt(key, sub, hex_), (label, pos, value)
    assert len(flagged) >= len(positions) * (256 - 66)
    for pos, value in flagged[::37]:
        t = we.substitute(text, pos, value)
        try:
            want = we.ref_decrypt(key, t, hex_)
        except ValueError as e:  # binascii.Error and UnicodeDecodeError are ValueErrors
            with pytest.raises(type(e)):
                aes.decrypt_vec(key, stage(t), hex=hex_)
            continue
        assert host(aes.decrypt_vec(key, stage(t), hex=hex_)) == want, (label, pos, value)


# ---------------------------------------------------------------- 5. guard bands
@pytest.mark.parametrize("hex_", [False, True])
def test_encrypt_writes_nothing_outside_its_text(hex_):
    key, nonce = KEYS[0], NONCES[1]
    for total in (3071, 3072, 3073, 6143, 6144, 6145):
        n = total - 16
        if total == 6144:
            assert we.enc_wave_full(n, 1) and we.enc_units(n) == 128  # the last store is a coalesced one
        data = stage(we.rand_bytes(n, total))
        need = aes.encrypt_buffer(n, hex_, dev()).numel()
        buf = torch.full((need + 64,), CANARY, dtype=torch.uint8, device=dev())
        got = aes.encrypt_vec(key, data, nonce=nonce, hex=hex_, out=buf)
        want = (b"0x" if hex_ else b"") + we.want_text(key, nonce, host(data), hex_)
        assert host(got) == want, total
        assert need == (16 if hex_ else 0) + we.text_len(n, hex_)
        assert host(buf[need:]) == bytes([CANARY]) * 64, total
        if hex_:
            assert host(buf[:14]) == bytes([CANARY]) * 14 and host(buf[14:16]) == b"0x", total


def test_ctr_writes_nothing_at_or_after_n():
    key, nonce = KEYS[0], NONCES[3]
    for n in (16, 17, 31, 4096, 4097, 4111):
        data = we.rand_bytes(n, n)
        out = torch.full((n + 64,), CANARY, dtype=torch.uint8, device=dev())
        aes.ctr_vec(key, nonce, stage(data), out=out)
        assert host(out[:n]) == c_oracle.aes_ctr(key, nonce, data), n
        assert host(out[n:]) == bytes([CANARY]) * 64, n


@pytest.mark.parametrize("lib", LAYOUTS)
def test_decrypt_writes_nothing_at_or_after_its_capacity(lib, monkeypatch):
    key, nonce = KEYS[0], NONCES[0]
    with layout(lib, monkeypatch):
        for n in (0, 1, 2, 47, 3056, 6127, 6128, 6129, we.n_for_units(66, 4), we.n_for_units(130, 5)):
            data = we.rand_bytes(n, n + 1)
            for hex_ in (False, True):
                text = we.want_text(key, nonce, data, hex_)
                cap = we.plain_capacity(len(text), hex_)
                rc, out, out_len, bad = raw_decrypt(key, stage(text), hex_, slack=64)
                assert (rc, bad, out_len) == (0, 0, n) and host(out[:n]) == data, (n, hex_)
                assert host(out[cap:cap + 64]) == bytes([CANARY]) * 64, (n, hex_)
