"""resolve_records_vec on the host side (no kernel launches).

* the method, the binding and the C entry point exist, and the symbol is
  listed in _native.EXPORTS;
* every argument error of the method fires before any device use (CPU
  tensors, no HIP device needed), with resolve_shares_vec's messages and
  exception types where the check is resolve_shares_vec's;
* dn_m521_reconstruct_records validates before any device call: n_elem == 0 is
  DN_OK and touches no pointer; a null pointer, a wire that is not 4-byte
  aligned, k = 1 and k = 17, malformed weights and no output are DN_ERR_ARG.

(That wire_edges.decode_window predicts which waves take the byte-serial path
is test_wire_geom_host.py's: the window geometry is csrc/wire_geom.hpp's for
every kernel.)
"""
import ctypes
import os

import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native, codec



def test_method_binding_and_entry_point_exist():
    assert callable(getattr(shamir.SecretShare, "resolve_records_vec"))
    assert callable(_native.reconstruct_records)
    assert callable(codec.check_bad_records)
    assert hasattr(_native.lib(), "dn_m521_reconstruct_records")
    assert "dn_m521_reconstruct_records" in _native.EXPORTS
    assert "dn_m521_reconstruct_records" in _native.exported_symbols()


def _wires(k, n=4, **kw):
    return [(torch.zeros(8 * n, dtype=torch.uint8, **kw), torch.zeros(n + 1, dtype=torch.int64, **kw))
            for _ in range(k)]


def test_argument_errors_fire_before_any_device_use(monkeypatch):
    def no_device():
        raise AssertionError("resolve_records_vec reached the device before its argument checks")

    monkeypatch.setattr(_native, "require_device", no_device)
    monkeypatch.setattr(_native, "reconstruct_records", lambda *a, **k: no_device())
    r = shamir.SecretShare(3).resolve_records_vec
    with pytest.raises(NotImplementedError, match="GF\\(2\\^521 - 1\\) only"):
        shamir.SecretShare(3, prime=(1 << 127) - 1).resolve_records_vec([], [], 4)  # _require_m521 comes first
    # resolve_shares_vec's checks, messages and types
    with pytest.raises(ValueError, match="^not enough values to unpack \\(expected 2, got 0\\)$"):
        r([], [], 4)
    with pytest.raises(ValueError, match="^not enough values to unpack \\(expected 2, got 0\\)$"):
        r([], None, 4)
    with pytest.raises(ValueError, match="^need at least 3 shares$"):
        r(_wires(2), [1, 2], 4)
    with pytest.raises(ValueError, match="^shares must be distinct$"):
        r(_wires(3), [1, 2, 1], 4)
    with pytest.raises(TypeError, match="^reduce\\(\\) of empty iterable with no initial value$"):
        shamir.SecretShare(1).resolve_records_vec(_wires(1), [7], 4)
    with pytest.raises(ValueError, match="^resolve_records_vec: one abscissa per wire$"):
        r(_wires(3), [1, 2], 4)
    with pytest.raises(ValueError, match='out must be "int64" or "field"'):
        r(_wires(3), [1, 2, 3], 4, out="bytes")
    # the pairs themselves
    with pytest.raises(ValueError, match="records must be \\(packed, offsets\\) pairs"):
        r([(torch.zeros(4, dtype=torch.uint8),)] * 3, [1, 2, 3], 4)
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
        with pytest.raises(ValueError, match="resolve_records_vec: .*" + what):
            r(good + [bad_pair], [1, 2, 3], 4)
    with pytest.raises(ValueError, match="n must not be negative"):
        r(_wires(3), [1, 2, 3], -1)
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64),
                torch.zeros(4, dtype=torch.int32)[::2], [0, 0], torch.zeros(2, dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="bad must be a contiguous int32 tensor \\[2\\]"):
            r(_wires(3), [1, 2, 3], 4, bad=bad)
    with pytest.raises(ValueError, match="xs=None needs a first record"):
        r(_wires(3, n=0), None, 0)


def test_the_device_is_required_only_after_the_checks(monkeypatch):
    """Valid CPU arguments get as far as the device requirement, and no further."""
    class Reached(Exception):
        pass

    def reached():
        raise Reached

    monkeypatch.setattr(_native, "require_device", reached)
    monkeypatch.setattr(_native, "reconstruct_records", lambda *a, **k: pytest.fail("launched"))
    with pytest.raises(Reached):
        shamir.SecretShare(3).resolve_records_vec(_wires(3), [1, 3, 5], 4, bad=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(Reached):
        shamir.SecretShare(2).resolve_records_vec(_wires(17), None, 4, out="field", return_overflow=True)


def test_binding_checks_its_counts():
    w = _native.lagrange([1, 3, 5], 3)
    with pytest.raises(ValueError, match="one wire and one abscissa per weight"):
        _native.reconstruct_records([(4096, 8, 8192)] * 2, [1, 3], w, None, n=1)
    with pytest.raises(ValueError, match="one wire and one abscissa per weight"):
        _native.reconstruct_records([(4096, 8, 8192)] * 3, [1, 3], w, None, n=1)


def test_check_bad_records_names_both_counts():
    codec.check_bad_records(torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="^resolve_records_vec: 3 records with x > 8 bytes or y > 68 bytes, "
                                         "0 records whose x is not their wire's abscissa$"):
        codec.check_bad_records(torch.tensor([3, 0], dtype=torch.int32))
    with pytest.raises(ValueError, match="0 records with .*, 2 records whose x is not"):
        codec.check_bad_records(torch.tensor([0, 2], dtype=torch.int32))


def test_entry_point_validates_before_any_device_call():
    f = _native.lib().dn_m521_reconstruct_records
    OK, ARG = _native.DN_OK, _native.DN_ERR_ARG
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    base = 0x7F0000000000  # never dereferenced: every call below returns before a launch
    w = _native.lagrange([1, 3, 5], 3)
    wp = ctypes.byref(w)

    def ptrs(*p):
        return (vp * len(p))(*p)

    ins, offs = ptrs(base, base + 4096, base + 8192), ptrs(base + (1 << 20), base + (2 << 20), base + (3 << 20))
    nb, xs = (u64 * 3)(64, 64, 64), (u64 * 3)(1, 3, 5)
    # n_elem == 0: DN_OK whatever else is passed, no pointer touched
    assert f(None, None, None, None, None, None, None, None, None, 0, None) == OK
    assert f(ptrs(None, None, None), nb, offs, xs, wp, None, None, None, None, 0, None) == OK
    # null pointers
    for args in [(None, nb, offs, xs, wp, base, base, None, base), (ins, None, offs, xs, wp, base, base, None, base),
                 (ins, nb, None, xs, wp, base, base, None, base), (ins, nb, offs, None, wp, base, base, None, base),
                 (ins, nb, offs, xs, None, base, base, None, base), (ins, nb, offs, xs, wp, base, base, None, None)]:
        assert f(*args, 5, None) == ARG
        assert "null pointer" in _native.last_error()
    assert f(ins, nb, offs, xs, wp, None, None, None, base, 5, None) == ARG
    assert "no output" in _native.last_error()
    assert f(ptrs(base, None, base), nb, offs, xs, wp, base, None, None, base, 5, None) == ARG
    assert "null wire 1" in _native.last_error()
    assert f(ins, nb, ptrs(base, base, None), xs, wp, base, None, None, base, 5, None) == ARG
    assert "null wire 2" in _native.last_error()
    # a wire that is not 4-byte aligned (wires may differ: 4 and 16 are both fine, 1..3 are not)
    for skew in (1, 2, 3):
        assert f(ptrs(base, base + 4096 + skew, base + 8196), nb, offs, xs, wp, None, base, None, base, 5, None) == ARG
        assert "wire 1 must be 4-byte aligned" in _native.last_error()
    # k outside 2..16
    for k in (0, 1, 17):
        bad = _native.lagrange([1, 3, 5], 3)
        bad.k = k
        assert f(ins, nb, offs, xs, ctypes.byref(bad), base, base, None, base, 5, None) == ARG
        assert f"k={k} outside 2..16" in _native.last_error()
    bad = _native.lagrange([1, 3, 5], 3)
    bad.a_limbs = 5
    assert f(ins, nb, offs, xs, ctypes.byref(bad), base, base, None, base, 5, None) == ARG
    assert "malformed weights" in _native.last_error()
    bad = _native.lagrange([2, 4, 5], 3)
    assert bad.has_inv == 2
    bad.d = 4
    assert f(ins, nb, offs, xs, ctypes.byref(bad), base, base, None, base, 5, None) == ARG
    assert "malformed divisor" in _native.last_error()
