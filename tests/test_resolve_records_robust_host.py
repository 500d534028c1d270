"""resolve_records_vec_robust on the host side (no kernel launches): the method, the binding and the
entry point exist; every argument rule fires before any device use with the neighbouring calls' types
and messages; dn_m521_reconstruct_records_robust validates before any device call."""
import ctypes

import pytest
import torch

from delta_node.crypto import shamir
from delta_node.crypto.shamir import _native

XS5 = [1, 2, 3, 4, 5]
FLAGS = [torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)[::2]]


def _wires(k, n=4):
    return [(torch.zeros(8 * n, dtype=torch.uint8), torch.zeros(n + 1, dtype=torch.int64)) for _ in range(k)]


def _strided(k):
    return _wires(k - 1) + [(torch.zeros(32, dtype=torch.uint8), torch.zeros(10, dtype=torch.int64)[::2])]


def test_method_binding_and_entry_point_exist():
    assert callable(getattr(shamir.SecretShare, "resolve_records_vec_robust"))
    assert callable(_native.reconstruct_records_robust)
    assert hasattr(_native.lib(), "dn_m521_reconstruct_records_robust")
    assert "dn_m521_reconstruct_records_robust" in _native.EXPORTS


@pytest.mark.parametrize("t, wires, xs, kw, exc, text", [
    (3, _wires(4), [1, 2, 3, 4], {}, NotImplementedError, "one spare share detects only"),
    (3, _wires(5), [3, 8, 17, 26, 37], {}, NotImplementedError, "odd part of 2\\^16 or more"),
    (13, _wires(17), list(range(1, 18)), {}, NotImplementedError, "more than 16 shares"),
    (3, _wires(5), [1, 2, 3, 4, 1 << 64], {}, NotImplementedError,
     "^resolve_records_vec_robust: abscissas must fit 64 bits$"),
    (3, _wires(5), XS5, {"out": "int32"}, ValueError, '^resolve_records_vec_robust: out must be "int64" or "field"$'),
    (3, _wires(5), [1, 2, 3, 4], {}, ValueError, "^resolve_records_vec_robust: one abscissa per wire$"),
    (3, _wires(5), [1, 2, 3, 4, 1], {}, ValueError, "^shares must be distinct$"),
    (3, _strided(5), XS5, {}, ValueError, "offsets must be contiguous"),
] + [(3, _wires(5), XS5, {"bad": f}, ValueError,
      "^resolve_records_vec_robust: bad must be a contiguous int32 tensor \\[2\\]") for f in FLAGS]
  + [(3, _wires(5), XS5, {"bad_records": f}, ValueError,
      "^resolve_records_vec_robust: bad_records: bad must be a contiguous int32 tensor \\[2\\]") for f in FLAGS])
def test_argument_rules_fire_before_any_device_use(monkeypatch, t, wires, xs, kw, exc, text):
    def no_device(*a, **k):
        raise AssertionError("resolve_records_vec_robust reached the device before its argument checks")

    monkeypatch.setattr(_native, "require_device", no_device)
    monkeypatch.setattr(_native, "reconstruct_records_robust", no_device)
    with pytest.raises(exc, match=text):
        shamir.SecretShare(t).resolve_records_vec_robust(wires, xs, 4, **kw)


def test_entry_point_validates_before_any_device_call():
    f = _native.lib().dn_m521_reconstruct_records_robust
    OK, ARG = _native.DN_OK, _native.DN_ERR_ARG
    base = 0x7F0000000000  # never dereferenced: every call below returns before a launch
    plan = _native.robust_plan(XS5, 3)
    pp = ctypes.byref(plan)
    ins = (ctypes.c_void_p * 5)(*[base + 4096 * i for i in range(5)])
    offs = (ctypes.c_void_p * 5)(*[base + ((i + 1) << 20) for i in range(5)])
    nb, xs = (ctypes.c_uint64 * 5)(*[64] * 5), (ctypes.c_uint64 * 5)(*XS5)
    assert f(None, None, None, None, None, None, None, None, None, None, 0, None) == OK
    for args, text in [((ins, nb, offs, xs, None, base, None, base, None, base), "null pointer"),
                       ((ins, nb, offs, xs, pp, base, None, None, None, base), "null pointer"),
                       ((ins, nb, offs, xs, pp, base, None, base, None, None), "null pointer"),
                       ((ins, nb, offs, xs, pp, None, None, base, None, base), "exactly one of out_fe and out_u64"),
                       ((ins, nb, offs, xs, pp, base, base, base, None, base), "exactly one of out_fe and out_u64")]:
        assert f(*args, 5, None) == ARG and text in _native.last_error()
    skew = (ctypes.c_void_p * 5)(base, base + 4098, base, base, base)
    assert f(skew, nb, offs, xs, pp, base, None, base, None, base, 5, None) == ARG
    assert "wire 1 must be 4-byte aligned" in _native.last_error()
    broken = _native.robust_plan(XS5, 3)
    broken.check.k = 17
    assert f(ins, nb, offs, xs, ctypes.byref(broken), base, None, base, None, base, 5, None) == ARG
    assert "malformed plan" in _native.last_error()
    assert f(ins, nb, offs, xs, pp, base, None, base, None, base, 1 << 39, None) == ARG
    assert "2^31 workgroups or more" in _native.last_error()
