"""The codec wrappers' cached device state belongs to one thread (no GPU).

`codec._scratch` hands the multi-launch entry points (dn_m521_encode_shares,
dn_m521_encode_shares_many, dn_m521_frame_open) the buffer their launches pass
lengths, tables and totals through, and the checked form of `decode_share_vec`
zeroes, fills and reads one cached counter.  ctypes enters those entry points
with the GIL released, so two threads on one stream interleave their launches:
a buffer or counter they shared would carry one call's state into the other's
launches.  The caches are therefore keyed by the calling thread as well as by
(device, stream) — pinned here on CPU tensors with the stream held constant;
tests/test_gpu_shared_state.py runs the calls themselves from four threads.
"""
import threading

import torch

from delta_node.crypto.shamir import _native, codec

CPU = torch.device("cpu")


def from_two_threads(fn):
    """[fn(), fn()] from each of two threads that are alive at the same time."""
    got, errs = [None, None], []
    barrier = threading.Barrier(2)

    def work(i):
        try:
            barrier.wait(timeout=30)
            first = fn()
            barrier.wait(timeout=30)  # both threads hold their first result before either asks again
            got[i] = [first, fn()]
        except BaseException as e:  # noqa: BLE001 (reported by the asserting thread)
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not any(th.is_alive() for th in threads) and not errs, errs
    return got


def storage(t) -> int:
    return t.untyped_storage().data_ptr()


def test_scratch_is_cached_per_thread(monkeypatch):
    monkeypatch.setattr(_native, "stream_ptr", lambda: 0x5EED)
    calls = threading.local()

    def ask():  # per thread: a size, then a smaller one that fits
        calls.n = getattr(calls, "n", 0) + 1
        return codec._scratch(CPU, 4096 if calls.n == 1 else 1000)

    a, b = from_two_threads(ask)
    for first, second in (a, b):
        assert first.dtype == torch.uint8 and first.numel() >= 1000
        assert second is first  # the same thread, a size that fits: the same tensor, nothing allocated
    assert storage(a[0]) != storage(b[0])  # two threads, one device and stream: two buffers
    mine = codec._scratch(CPU, 16)
    assert storage(mine) not in (storage(a[0]), storage(b[0]))  # and the asserting thread has its own
    assert codec._scratch(CPU, 16) is mine
    grown = codec._scratch(CPU, mine.numel() + 1)  # too small: replaced, and the new one is kept
    assert grown is not mine and grown.numel() >= mine.numel() + 1 and codec._scratch(CPU, 16) is grown


def test_scratch_is_still_keyed_by_stream(monkeypatch):
    monkeypatch.setattr(_native, "stream_ptr", lambda: 0x1000)
    one = codec._scratch(CPU, 64)
    monkeypatch.setattr(_native, "stream_ptr", lambda: 0x2000)
    other = codec._scratch(CPU, 64)
    assert storage(one) != storage(other) and codec._scratch(CPU, 64) is other
    monkeypatch.setattr(_native, "stream_ptr", lambda: 0x1000)
    assert codec._scratch(CPU, 64) is one


def test_checked_decode_flag_is_cached_per_thread(monkeypatch):
    monkeypatch.setattr(_native, "stream_ptr", lambda: 0x5EED)

    def ask():
        flag = codec._checked_flag(CPU)
        assert flag.dtype == torch.int32 and flag.tolist() == [0]
        flag += 3  # what a decode of three bad records leaves behind
        return flag

    a, b = from_two_threads(ask)
    for first, second in (a, b):
        assert second is first and second.tolist() == [3]  # zeroed again by the second request, then counted into
    assert storage(a[0]) != storage(b[0])  # one thread's zero_() cannot erase the other's count
