"""check_records_vec on the host side (no kernel launches).

* the method, the binding and the C entry point exist, and the symbol is
  listed in _native.EXPORTS;
* every argument error of the method fires before any device use (CPU
  tensors, no HIP device needed), with resolve_records_vec's messages and
  exception types where the check is resolve_records_vec's, and
  check_shares_vec's limits as NotImplementedError;
* dn_m521_check_records validates before any device call: n_elem == 0 is DN_OK
  and touches no pointer; a null pointer, a malformed plan, a wire that is not
  4-byte aligned and offsets that are not 8-byte aligned are DN_ERR_ARG.
"""
import ctypes

import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native


def test_method_binding_and_entry_point_exist():
    assert callable(getattr(shamir.SecretShare, "check_records_vec"))
    assert callable(_native.check_records)
    assert hasattr(_native.lib(), "dn_m521_check_records")
    assert "dn_m521_check_records" in _native.EXPORTS
    assert "dn_m521_check_records" in _native.exported_symbols()


def _wires(k, n=4, **kw):
    return [(torch.zeros(8 * n, dtype=torch.uint8, **kw), torch.zeros(n + 1, dtype=torch.int64, **kw))
            for _ in range(k)]


def test_argument_errors_fire_before_any_device_use(monkeypatch):
    def no_device():
        raise AssertionError("check_records_vec reached the device before its argument checks")

    monkeypatch.setattr(_native, "require_device", no_device)
    monkeypatch.setattr(_native, "check_records", lambda *a, **k: no_device())
    c = shamir.SecretShare(3).check_records_vec
    with pytest.raises(NotImplementedError, match="GF\\(2\\^521 - 1\\) only"):
        shamir.SecretShare(3, prime=(1 << 127) - 1).check_records_vec([], [], 4)
    with pytest.raises(ValueError, match="^not enough values to unpack \\(expected 2, got 0\\)$"):
        c([], [], 4)
    with pytest.raises(ValueError, match="^not enough values to unpack \\(expected 2, got 0\\)$"):
        c([], None, 4)
    with pytest.raises(ValueError, match="^check_records_vec: one abscissa per wire$"):
        c(_wires(5), [1, 2, 3, 4], 4)
    with pytest.raises(ValueError, match="^need at least 3 shares$"):
        c(_wires(2), [1, 2], 4)
    with pytest.raises(ValueError, match="^shares must be distinct$"):
        c(_wires(5), [1, 2, 3, 4, 1], 4)
    with pytest.raises(TypeError, match="^reduce\\(\\) of empty iterable with no initial value$"):
        shamir.SecretShare(1).check_records_vec(_wires(1), [7], 4)
    with pytest.raises(ValueError, match="records must be \\(packed, offsets\\) pairs"):
        c([(torch.zeros(4, dtype=torch.uint8),)] * 5, [1, 2, 3, 4, 5], 4)
    with pytest.raises(ValueError, match="check_records_vec: offsets must hold n \\+ 1 = 6 entries, got 5"):
        c(_wires(5), [1, 2, 3, 4, 5], 5)
    with pytest.raises(ValueError, match="check_records_vec: n must not be negative"):
        c(_wires(5), [1, 2, 3, 4, 5], -1)
    with pytest.raises(ValueError, match="xs=None needs a first record"):
        c(_wires(5, n=0), None, 0)
    # check_shares_vec's limits: NotImplementedError, no decode fallback
    for xs, text in [([1, 2, 3], "no spare share"), ([0, 1, 2, 3], "abscissa 0"),
                     ([1, 2, 3, 1 << 64], "check_records_vec: abscissas must fit 64 bits"),
                     (list(range(1, 9)), "more than 4 spare shares"), (list(range(1, 18)), "more than 16 shares")]:
        with pytest.raises(NotImplementedError, match=text):
            c(_wires(len(xs)), xs, 4)
    with pytest.raises(NotImplementedError, match="2\\^32 or more"):
        shamir.SecretShare(2).check_records_vec(_wires(4), [1, 2, 3, 100000], 4)
    # the two flags
    for flag in (torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64),
                 torch.zeros(4, dtype=torch.int32)[::2], [0, 0], torch.zeros(2, dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="^check_records_vec: bad must be a contiguous int32 tensor \\[2\\]"):
            c(_wires(5), [1, 2, 3, 4, 5], 4, bad=flag)
        with pytest.raises(ValueError, match="^check_records_vec: bad_records: bad must be a contiguous int32 "
                                             "tensor \\[2\\]"):
            c(_wires(5), [1, 2, 3, 4, 5], 4, bad_records=flag)


def test_the_device_is_required_only_after_the_checks(monkeypatch):
    """Valid CPU arguments get as far as the device requirement, and no further."""
    class Reached(Exception):
        pass

    def reached():
        raise Reached

    monkeypatch.setattr(_native, "require_device", reached)
    monkeypatch.setattr(_native, "check_records", lambda *a, **k: pytest.fail("launched"))
    flag = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(Reached):
        shamir.SecretShare(3).check_records_vec(_wires(5), [1, 2, 3, 4, 5], 4, culprit=True, bad=flag, bad_records=flag)
    with pytest.raises(Reached):
        shamir.SecretShare(2).check_records_vec(_wires(17), None, 4)


def test_binding_checks_its_counts():
    plan = _native.check_plan([1, 2, 3, 4, 5], 3)
    for wires, xs in [([(4096, 8, 8192)] * 4, [1, 2, 3, 4]), ([(4096, 8, 8192)] * 5, [1, 2, 3, 4])]:
        with pytest.raises(ValueError, match="one wire and one abscissa per share of the plan"):
            _native.check_records(wires, xs, plan, None, None, n=1)


def test_entry_point_validates_before_any_device_call():
    f = _native.lib().dn_m521_check_records
    OK, ARG = _native.DN_OK, _native.DN_ERR_ARG
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    base = 0x7F0000000000  # never dereferenced: every call below returns before a launch
    plan = _native.check_plan([1, 2, 3, 4], 3)
    pp = ctypes.byref(plan)

    def ptrs(*p):
        return (vp * len(p))(*p)

    ins = ptrs(*[base + 4096 * i for i in range(4)])
    offs = ptrs(*[base + ((i + 1) << 20) for i in range(4)])
    nb, xs = (u64 * 4)(64, 64, 64, 64), (u64 * 4)(1, 2, 3, 4)
    # n_elem == 0: DN_OK whatever else is passed, no pointer touched
    assert f(None, None, None, None, None, None, None, None, 0, None) == OK
    assert f(ptrs(None, None, None, None), nb, offs, xs, pp, None, None, None, 0, None) == OK
    # null pointers (culprit alone may be null)
    for args in [(None, nb, offs, xs, pp, base, None, base), (ins, None, offs, xs, pp, base, None, base),
                 (ins, nb, None, xs, pp, base, None, base), (ins, nb, offs, None, pp, base, None, base),
                 (ins, nb, offs, xs, None, base, None, base), (ins, nb, offs, xs, pp, None, None, base),
                 (ins, nb, offs, xs, pp, base, base, None)]:
        assert f(*args, 5, None) == ARG
        assert "null pointer" in _native.last_error()
    assert f(ptrs(base, None, base, base), nb, offs, xs, pp, base, None, base, 5, None) == ARG
    assert "null wire 1" in _native.last_error()
    assert f(ins, nb, ptrs(base, base, base, None), xs, pp, base, None, base, 5, None) == ARG
    assert "null wire 3" in _native.last_error()
    for skew in (1, 2, 3):
        assert f(ptrs(base, base + 4096 + skew, base, base), nb, offs, xs, pp, base, None, base, 5, None) == ARG
        assert "wire 1 must be 4-byte aligned" in _native.last_error()
    assert f(ins, nb, ptrs(base, base, base + 4, base), xs, pp, base, None, base, 5, None) == ARG
    assert "offsets of wire 2 must be 8-byte aligned" in _native.last_error()
    for field_name, value in (("k", 17), ("r", 5), ("r", 0)):
        broken = _native.check_plan([1, 2, 3, 4], 3)
        setattr(broken, field_name, value)
        assert f(ins, nb, offs, xs, ctypes.byref(broken), base, None, base, 5, None) == ARG
        assert "malformed plan" in _native.last_error()
    assert f(ins, nb, offs, xs, pp, base, None, base, 1 << 39, None) == ARG
    assert "2^31 workgroups or more" in _native.last_error()
