"""tests/scratch_guard.py proves itself on CPU tensors: planted violations are caught, a well-behaved entry passes, sizes
and alignment equal sfgs._call.scratch's, and nothing stays patched."""
import pytest
import torch

import scratch_guard
from scratch_guard import GUARD, GuardViolation, ScratchGuard
from sfgs import _call

CPU = torch.device("cpu")


# ---- stand-in "entries": what a wrapper does around a library call, with the kernel written in torch --------------------
def entry_well_behaved(n):
    s = _call.scratch(n, CPU)
    s.fill_(7)                              # writes all of its scratch, then reads it
    return int(s.sum())


def entry_writes_behind(n, offset):
    s = _call.scratch(n, CPU)
    s.fill_(0)
    base = torch.empty(0, dtype=torch.uint8).set_(s.untyped_storage(), 0, (s.untyped_storage().nbytes(),))
    base[s.storage_offset() + n + offset] = 1     # one byte at `offset` from the body's end (negative: before it)
    return 0


def entry_reads_unwritten(n):
    s = _call.scratch(n, CPU)
    total = int(s.to(torch.int64).sum())    # a counter nobody cleared
    s.fill_(0)
    return total


def entry_rasterizer_like(n):
    import diff_gauss
    t = diff_gauss.torch                    # torch as diff_gauss sees it
    blob = t.empty(n, dtype=t.uint8, device=CPU)
    other = t.empty(n, dtype=t.float32, device=CPU)
    two_d = t.empty(2, n, dtype=t.uint8, device=CPU)
    return blob, other, two_d


@pytest.mark.parametrize("offset, side", [(0, "after"), (5, "after"), (GUARD - 1, "after"), (-101, "before"), (-100 - GUARD, "before")])
def test_write_outside_the_body_is_caught(monkeypatch, offset, side):
    n = 100
    with ScratchGuard(monkeypatch, fill=0x00, device="cpu") as sg:
        entry_writes_behind(n, offset)
        assert sg.violations() == [(f"{__name__}.entry_writes_behind", side, offset, offset, n)]
        with pytest.raises(GuardViolation) as e:
            sg.check()
    msg = str(e.value)
    assert f"{__name__}.entry_writes_behind" in msg and f"guard {side}" in msg and f"{offset:+d}" in msg and "100 bytes requested" in msg


def test_first_and_last_changed_offset(monkeypatch):
    with ScratchGuard(monkeypatch, fill=0xFF, device="cpu") as sg:
        entry_writes_behind(64, 3)
        h = sg.handed[0]
        h.backing[h.start + 64 + 40] = 9
        assert sg.violations() == [(f"{__name__}.entry_writes_behind", "after", 3, 40, 64)]


def test_read_of_unwritten_scratch_depends_on_the_fill(monkeypatch):
    got = {}
    for fill in (0x00, 0xFF, 0xA5):
        with ScratchGuard(monkeypatch, fill=fill, device="cpu") as sg:
            got[fill] = entry_reads_unwritten(33)
            sg.check()
    assert got == {0x00: 0, 0xFF: 33 * 0xFF, 0xA5: 33 * 0xA5}


def test_well_behaved_entry_passes_and_is_fill_independent(monkeypatch):
    got = []
    for fill in (0x00, 0xFF, 0xA5):
        with ScratchGuard(monkeypatch, fill=fill, device="cpu") as sg:
            got.append(entry_well_behaved(1000))
            sg.check()
            assert len(sg.handed) == 1 and sg.handed[0].entry == f"{__name__}.entry_well_behaved"
    assert got == [7000] * 3 == [entry_well_behaved(1000)] * 3


@pytest.mark.parametrize("nbytes", [0, 1, 2, 511, 512, 513, 4097, 100_000])
def test_sizes_and_alignment_equal_call_scratch(monkeypatch, nbytes):
    own = _call.scratch(nbytes, CPU)
    with ScratchGuard(monkeypatch, fill=0xA5, device="cpu") as sg:
        s = _call.scratch(nbytes, CPU)
    assert (s.shape, s.dtype, s.device, s.is_contiguous()) == (own.shape, own.dtype, own.device, True)
    assert s.numel() == max(nbytes, 1) and s.data_ptr() % 512 == 0
    assert bool((s == 0xA5).all())
    h = sg.handed[0]
    assert h.backing.numel() >= 2 * GUARD + s.numel() and h.start >= GUARD
    assert bool((h.backing[h.start - GUARD:h.start] == scratch_guard.SENTINEL).all())
    assert bool((h.backing[h.start + s.numel():h.start + s.numel() + GUARD] == scratch_guard.SENTINEL).all())


def test_refused_if_zero_is_call_scratch_s(monkeypatch):
    class _Lib:
        @staticmethod
        def sfgs_last_error():
            return b"planted refusal"
    monkeypatch.setattr(_call.L, "load", lambda: _Lib)
    with pytest.raises(RuntimeError) as own:
        _call.scratch(0, CPU, refused_if_zero=True)
    with ScratchGuard(monkeypatch, fill=0, device="cpu") as sg:
        with pytest.raises(RuntimeError) as guarded:
            _call.scratch(0, CPU, refused_if_zero=True)
        assert _call.scratch(0, CPU).numel() == 1 and _call.scratch(8, CPU, refused_if_zero=True).numel() == 8
        assert len(sg.handed) == 2
    assert str(own.value) == str(guarded.value) == "libsfgs: planted refusal"


def test_short_hands_out_less_from_a_full_size_backing(monkeypatch):
    with ScratchGuard(monkeypatch, fill=0x11, device="cpu", short=1) as sg:
        a, b = _call.scratch(100, CPU), _call.scratch(1, CPU)
        assert a.numel() == 99 and b.numel() == 1          # nbytes > k only
        h = sg.handed[0]
        assert h.asked == 100 and h.backing.numel() >= 2 * GUARD + 100
        assert sg.short_tails_intact()
        h.backing[h.start + 99] = 0                        # a library that ignored the size: inside the backing, and seen
        assert not sg.short_tails_intact()
        sg.check()                                         # ... while the guards are intact


def test_short_for_one_entry_and_untouched_bodies(monkeypatch):
    def first(n):
        return _call.scratch(n, CPU)

    def second(n):
        return _call.scratch(n, CPU)
    with ScratchGuard(monkeypatch, fill=0x22, device="cpu", short=1, short_for="second") as sg:
        a, b = first(64), second(64)
        assert (a.numel(), b.numel()) == (64, 63)
        a.fill_(0)                                         # the call before the refused one ran: its body does not count
        assert sg.shortened_bodies_intact()
        b[5] = 1                                           # a refused call that launched something all the same
        assert not sg.shortened_bodies_intact()
    with ScratchGuard(monkeypatch, fill=0x22, device="cpu", short=1, short_for="nobody") as sg:
        assert first(64).numel() == 64 and not sg.shortened_bodies_intact()      # nothing was shortened: not a pass


def test_rasterizer_site_intercepts_1d_uint8_only(monkeypatch):
    import diff_gauss
    with ScratchGuard(monkeypatch, fill=0x5A, device="cpu") as sg:
        assert diff_gauss.torch is not torch and diff_gauss.torch.float32 is torch.float32
        blob, other, two_d = entry_rasterizer_like(300)
        assert [h.entry for h in sg.handed] == [f"{__name__}.entry_rasterizer_like"] and sg.handed[0].asked == 300
        assert blob.shape == (300,) and blob.dtype == torch.uint8 and bool((blob == 0x5A).all()) and blob.data_ptr() % 512 == 0
        assert other.dtype == torch.float32 and two_d.shape == (2, 300)
        sg.check()
    with ScratchGuard(monkeypatch, fill=0x5A, device="cuda") as sg:      # another device's allocations pass through
        entry_rasterizer_like(300)
        assert sg.handed == []


def test_nothing_stays_patched(monkeypatch):
    import diff_gauss
    own = (_call.scratch, diff_gauss.torch, torch.empty)
    with ScratchGuard(monkeypatch, fill=0, device="cpu"):
        assert _call.scratch is not own[0] and diff_gauss.torch is not torch
        assert torch.empty is own[2]                       # the global torch.empty is never touched
    assert (_call.scratch, diff_gauss.torch, torch.empty) == own and diff_gauss.torch is torch
    with pytest.raises(ZeroDivisionError):
        with ScratchGuard(monkeypatch, fill=0, device="cpu"):
            1 / 0
    assert (_call.scratch, diff_gauss.torch, torch.empty) == own
    assert _call.scratch(5, CPU).untyped_storage().nbytes() < GUARD   # the real allocation again
