"""sum_records_vec on the host side (no kernel launches).

* the method, the binding and the C entry point exist, and the symbol is
  listed in _native.EXPORTS;
* (that wire_edges.decode_window predicts which waves take the byte-serial
  path is test_wire_geom_host.py's: the window geometry is csrc/wire_geom.hpp's
  for every kernel);
* every argument error of the method fires before any device use (CPU
  tensors, no HIP device needed), and valid CPU arguments reach the device
  requirement and go no further;
* dn_m521_sum_records validates before any device call: n_elem == 0 is DN_OK
  and touches no pointer; m == 0, a null pointer, a wire that is not 4-byte
  aligned, offsets that are not 8-byte aligned, 2^31 tiles and an `acc` that
  overlaps `out` are DN_ERR_ARG, the wire named where one is at fault;
* codec.check_bad_records names the method it is told.

The chaining of more than DN_M521_SUM_RECORDS_GROUP wires is a plain loop in
the entry point (launch j takes wires [j G, (j + 1) G) and accumulates into
`out`): there is no plan header, hence no stand-alone host program.
"""
import ctypes
import os
import re

import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, codec, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_method_binding_and_entry_point_exist():
    assert callable(getattr(shamir.SecretShare, "sum_records_vec"))
    assert callable(_native.sum_records)
    assert hasattr(_native.lib(), "dn_m521_sum_records")
    assert "dn_m521_sum_records" in _native.EXPORTS
    assert "dn_m521_sum_records" in _native.exported_symbols()


def group() -> int:
    """DN_M521_SUM_RECORDS_GROUP as include/dn_shamir.h defines it."""
    with open(os.path.join(ROOT, "include", "dn_shamir.h")) as f:
        found = re.findall(r"^#define DN_M521_SUM_RECORDS_GROUP (\d+)$", f.read(), flags=re.M)
    assert len(found) == 1, found
    return int(found[0])


def test_group_constant_holds_whole_sign_words():
    assert group() % 32 == 0 and group() >= 32


def _wires(m, n=4, **kw):
    return [(torch.zeros(8 * n, dtype=torch.uint8, **kw), torch.zeros(n + 1, dtype=torch.int64, **kw))
            for _ in range(m)]


def test_argument_errors_fire_before_any_device_use(monkeypatch):
    def no_device():
        raise AssertionError("sum_records_vec reached the device before its argument checks")

    monkeypatch.setattr(_native, "require_device", no_device)
    monkeypatch.setattr(_native, "sum_records", lambda *a, **k: no_device())
    r = shamir.SecretShare(3).sum_records_vec
    with pytest.raises(NotImplementedError, match="GF\\(2\\^521 - 1\\) only"):
        shamir.SecretShare(3, prime=(1 << 127) - 1).sum_records_vec(_wires(2), 1, 4)  # _require_m521 comes first
    with pytest.raises(ValueError, match="^sum_records_vec: no records$"):
        r([], 1, 4)
    with pytest.raises(ValueError, match="sum_records_vec: records must be \\(packed, offsets\\) pairs"):
        r([(torch.zeros(4, dtype=torch.uint8),)] * 3, 1, 4)
    good = _wires(2)
    p, o = _wires(1)[0]
    for bad_pair, what in [((p.to(torch.int8), o), "packed records must be contiguous 1-D uint8"),
                           ((torch.zeros(64, dtype=torch.uint8)[::2], o),
                            "packed records must be contiguous 1-D uint8"),
                           ((p.reshape(2, -1), o), "packed records must be contiguous 1-D uint8"),
                           ((bytes(32), o), "packed records must be contiguous 1-D uint8"),
                           ((p, o.to(torch.int32)), "offsets must be contiguous 1-D int64"),
                           ((p, torch.zeros(10, dtype=torch.int64)[::2]), "offsets must be contiguous 1-D int64"),
                           ((p, o.tolist()), "offsets must be contiguous 1-D int64"),
                           ((p, o[:4]), "offsets must hold n \\+ 1 = 5 entries, got 4"),
                           ((p.to("meta"), o), "must be on one device")]:
        with pytest.raises(ValueError, match="^sum_records_vec: .*" + what):
            r(good + [bad_pair], 1, 4)
    with pytest.raises(ValueError, match="sum_records_vec: n must not be negative"):
        r(_wires(3), 1, -1)
    # the abscissa
    for x in (-1, 1 << 64):
        with pytest.raises(ValueError, match="sum_records_vec: x must fit 64 bits"):
            r(_wires(3), x, 4)
    for x in (True, 1.0, "1"):
        with pytest.raises(ValueError, match="sum_records_vec: x must be an integer or None"):
            r(_wires(3), x, 4)
    with pytest.raises(ValueError, match="sum_records_vec: x=None needs a first record"):
        r(_wires(3, n=0), None, 0)
    # the signs: sum_shares_vec's rules
    with pytest.raises(ValueError, match="sum_records_vec: 2 signs for 3 wires"):
        r(_wires(3), 1, 4, signs=[1, -1])
    for signs in ([1, 0, 1], [1, True, 1], [1, -1.0, 1], [1, 2, 1], [1, "-1", 1]):
        with pytest.raises(ValueError, match="sum_records_vec: signs must be \\+1 or -1"):
            r(_wires(3), 1, 4, signs=signs)
    # acc / out
    vb = field.vec_bytes(4)
    ok = torch.zeros(vb, dtype=torch.uint8)
    for name in ("acc", "out"):
        for t in (torch.zeros(vb - 1, dtype=torch.uint8), torch.zeros(vb, dtype=torch.int8),
                  torch.zeros(2 * vb, dtype=torch.uint8)[::2], torch.zeros(1, vb, dtype=torch.uint8), bytes(vb),
                  torch.zeros(vb, dtype=torch.uint8, device="meta")):
            with pytest.raises(ValueError, match=f"sum_records_vec: {name} must be a contiguous uint8 tensor "
                                                 f"\\[{vb}\\]"):
                r(_wires(3), 1, 4, **{name: t, ("out" if name == "acc" else "acc"): ok})
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64),
                torch.zeros(4, dtype=torch.int32)[::2], [0, 0], torch.zeros(2, dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="sum_records_vec: bad must be a contiguous int32 tensor \\[2\\]"):
            r(_wires(3), 1, 4, bad=bad)


def test_the_device_is_required_only_after_the_checks(monkeypatch):
    """Valid CPU arguments get as far as the device requirement, and no further."""
    class Reached(Exception):
        pass

    def reached():
        raise Reached

    monkeypatch.setattr(_native, "require_device", reached)
    monkeypatch.setattr(_native, "sum_records", lambda *a, **k: pytest.fail("launched"))
    vb = field.vec_bytes(4)
    buf = torch.zeros(vb, dtype=torch.uint8)
    with pytest.raises(Reached):
        shamir.SecretShare(3).sum_records_vec(_wires(3), 3, 4, signs=[1, -1, 1], acc=buf, out=buf,
                                              bad=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(Reached):
        shamir.SecretShare(2).sum_records_vec(_wires(200), None, 4)
    with pytest.raises(Reached):  # n = 0 still asks for the device its empty result lives on
        shamir.SecretShare(2).sum_records_vec(_wires(1, n=0), 0, 0)


def test_binding_checks_its_counts():
    with pytest.raises(ValueError, match="sum_records: one negate flag per wire"):
        _native.sum_records([(4096, 8, 8192)] * 3, 1, [True, False], None, None, n=1)
    with pytest.raises(ValueError, match="sum_records: x must fit 64 bits"):
        _native.sum_records([(4096, 8, 8192)] * 3, 1 << 64, None, None, None, n=1)


def test_check_bad_records_names_the_method_it_is_told():
    codec.check_bad_records(torch.zeros(2, dtype=torch.int32), what="sum_records_vec")
    with pytest.raises(ValueError, match="^sum_records_vec: 3 records with x > 8 bytes or y > 68 bytes, "
                                         "1 records whose x is not their wire's abscissa$"):
        codec.check_bad_records(torch.tensor([3, 1], dtype=torch.int32), what="sum_records_vec")
    with pytest.raises(ValueError, match="^resolve_records_vec: 0 records with .*, 2 records whose x is not"):
        codec.check_bad_records(torch.tensor([0, 2], dtype=torch.int32))  # the default message stays


def test_entry_point_validates_before_any_device_call():
    f = _native.lib().dn_m521_sum_records
    OK, ARG = _native.DN_OK, _native.DN_ERR_ARG
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    base = 0x7F0000000000  # never dereferenced: every call below returns before a launch
    out, acc, bad = base + (8 << 20), base + (16 << 20), base + (24 << 20)

    def ptrs(*p):
        return (vp * len(p))(*p)

    ins, offs = ptrs(base, base + 4096, base + 8192), ptrs(base + (1 << 20), base + (2 << 20), base + (3 << 20))
    nb = (u64 * 3)(64, 64, 64)
    # n_elem == 0: DN_OK whatever else is passed, no pointer touched
    assert f(None, None, None, 0, 1, None, None, None, None, 0, None) == OK
    assert f(ptrs(None, None, None), nb, offs, 3, 1, None, None, None, None, 0, None) == OK
    # m == 0
    assert f(ins, nb, offs, 0, 1, None, None, out, bad, 5, None) == ARG
    assert "no wire" in _native.last_error()
    # null pointers
    for args in [(None, nb, offs, 3, 1, None, None, out, bad), (ins, None, offs, 3, 1, None, None, out, bad),
                 (ins, nb, None, 3, 1, None, None, out, bad), (ins, nb, offs, 3, 1, None, None, None, bad),
                 (ins, nb, offs, 3, 1, None, acc, out, None)]:
        assert f(*args, 5, None) == ARG
        assert "null pointer" in _native.last_error()
    assert f(ptrs(base, None, base), nb, offs, 3, 1, None, None, out, bad, 5, None) == ARG
    assert "null wire 1" in _native.last_error()
    assert f(ins, nb, ptrs(base, base, None), 3, 1, None, None, out, bad, 5, None) == ARG
    assert "null wire 2" in _native.last_error()
    # a wire that is not 4-byte aligned (wires may differ: 4 and 16 are both fine, 1..3 are not)
    for skew in (1, 2, 3):
        assert f(ptrs(base, base + 4096 + skew, base + 8196), nb, offs, 3, 1, None, None, out, bad, 5, None) == ARG
        assert "wire 1 must be 4-byte aligned" in _native.last_error()
    # offsets that are not 8-byte aligned
    for skew in (1, 4):
        assert f(ins, nb, ptrs(base + (1 << 20), base + (2 << 20), base + (3 << 20) + skew), 3, 1, None, None, out,
                 bad, 5, None) == ARG
        assert "offsets of wire 2 must be 8-byte aligned" in _native.last_error()
    # a wire at fault beyond the first launch's group is still found before anything is launched
    G = group()
    many_in = ptrs(*([base] * (G + 1) + [base + 2]))
    many_off = ptrs(*([base + (1 << 20)] * (G + 2)))
    assert f(many_in, (u64 * (G + 2))(*([64] * (G + 2))), many_off, G + 2, 1, None, None, out, bad, 5, None) == ARG
    assert f"wire {G + 1} must be 4-byte aligned" in _native.last_error()
    # 2^31 tiles or more
    assert f(ins, nb, offs, 3, 1, None, None, out, bad, 256 << 31, None) == ARG
    assert "2^31" in _native.last_error()
    assert f(ins, nb, offs, 3, 1, None, None, out, bad, (256 << 31) - 255, None) == ARG
    # acc may equal out; overlapping it otherwise is refused (5 elements: one 16896-byte tile)
    for delta in (1, 66, field.TILE_BYTES - 1, -1, -(field.TILE_BYTES - 1)):
        assert f(ins, nb, offs, 3, 1, None, out + delta, out, bad, 5, None) == ARG
        assert "acc overlaps out" in _native.last_error()
