"""Guard bands and chosen fills for the scratch blobs of libsfgs.so's wrappers (a plain helper, not a conftest).

    with ScratchGuard(monkeypatch, fill=0xA5) as sg:
        out = wrapper(...)        # every scratch blob it allocates is a view into [guard | body | guard]
        sg.check()                # synchronises; fails on the first guard byte that changed

Two allocation sites are swapped for the duration of the `with` block and nowhere else:
  * sfgs._call.scratch -- every wrapper except the rasterizer's gets its blob there and passes scratch.numel() on;
  * torch.empty AS diff_gauss SEES IT -- the module's global `torch` becomes a proxy whose `empty` intercepts
    one-dimensional uint8 allocations on the guarded device (the scratch blob and the dupgrad blob) and passes everything
    else through; every other attribute is torch's own. diff_gauss itself is not changed.

A body has exactly the length asked for (for _call.scratch: max(nbytes, 1); refused_if_zero as in the original) and
starts on a 512-byte boundary like torch.empty's. The guards hold SENTINEL, the body holds the test's fill byte: a kernel
that reads scratch words no kernel or memset of the call has written computes from 0x00, 0xFF or 0xA5 words instead of the
allocator's recycled (plausible) ones. `short=k` hands out nbytes - k bytes where nbytes > k, still carved from a
full-size backing: a library that ignored the size would write into the tail or the guard, never outside the backing buffer.
"""
import sys

import torch

GUARD = 64 * 1024
SENTINEL = 0xC3
ALIGN = 512


class GuardViolation(AssertionError):
    pass


class _Handed:
    __slots__ = ("backing", "start", "asked", "given", "entry")

    def __init__(self, backing, start, asked, given, entry):
        self.backing, self.start, self.asked, self.given, self.entry = backing, start, asked, given, entry

    @property
    def body(self):
        return self.backing[self.start:self.start + self.given]


class _TorchProxy:
    """`torch` with `empty` replaced; every other attribute is the real module's."""

    def __init__(self, guard):
        self._guard = guard

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        g = self._guard
        if (len(size) == 1 and isinstance(size[0], int) and kw.get("dtype") is torch.uint8
                and set(kw) <= {"dtype", "device"} and g._on_device(kw.get("device"))):
            return g._alloc(size[0], torch.device(kw["device"]), depth=2)
        return torch.empty(*size, **kw)


class ScratchGuard:
    def __init__(self, monkeypatch, fill, device="cuda", short=0, guard=GUARD, sentinel=SENTINEL, short_for=None):
        """short_for: shorten only the allocations of the entries whose name contains this text (an entry whose wrapper asks
        for scratch several times is then refused at the call under test, not at the first one)."""
        assert 0 <= fill <= 255 and 0 <= sentinel <= 255 and guard > 0 and guard % ALIGN == 0 and short >= 0
        self.monkeypatch, self.fill, self.short, self.guard, self.sentinel = monkeypatch, fill, short, guard, sentinel
        self.short_for = short_for
        self.device = torch.device(device)
        self.handed = []      # every buffer handed out, in order
        self._ctx = None

    # ---- the two patched sites ---------------------------------------------------------------------------------------
    def __enter__(self):
        from sfgs import _call
        import diff_gauss
        self._ctx = self.monkeypatch.context()
        m = self._ctx.__enter__()
        own_scratch = _call.scratch

        def scratch(nbytes, dev, refused_if_zero=False):
            if refused_if_zero and nbytes == 0:
                return own_scratch(nbytes, dev, refused_if_zero)     # raises the library's message, as the original does
            return self._alloc(max(int(nbytes), 1), torch.device(dev), depth=2)

        m.setattr(_call, "scratch", scratch)
        m.setattr(diff_gauss, "torch", _TorchProxy(self))
        return self

    def __exit__(self, *exc):
        ctx, self._ctx = self._ctx, None
        return ctx.__exit__(*exc)

    def _on_device(self, dev):
        if dev is None:
            return False
        dev = torch.device(dev)
        return dev.type == self.device.type and (self.device.index is None or dev.index in (None, self.device.index))

    def _alloc(self, nbytes, dev, depth):
        f = sys._getframe(depth)      # the function that asked: the wrapper (via _call.scratch) or diff_gauss's forward / backward
        entry = f"{f.f_globals.get('__name__', '?')}.{f.f_code.co_name}"
        # [slack to the 512-byte boundary | guard | body (asked bytes) | guard]
        backing = torch.empty(ALIGN + self.guard + nbytes + self.guard, dtype=torch.uint8, device=dev)
        start = (-backing.data_ptr()) % ALIGN + self.guard
        backing.fill_(self.sentinel)
        backing[start:start + nbytes].fill_(self.fill)
        shorten = nbytes > self.short and (self.short_for is None or self.short_for in entry)
        given = nbytes - self.short if shorten else nbytes
        h = _Handed(backing, start, nbytes, given, entry)
        self.handed.append(h)
        body = h.body
        assert body.data_ptr() % ALIGN == 0 and body.numel() == given
        return body

    # ---- the check ---------------------------------------------------------------------------------------------------
    def violations(self):
        """[(entry, side, first, last, asked)]: changed guard bytes, offsets relative to the END of the (full-size) body --
        "after" offsets are >= 0, "before" offsets are < -asked."""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        found = []
        for h in self.handed:
            end = h.start + h.asked
            for side, lo, hi in (("before", h.start - self.guard, h.start), ("after", end, end + self.guard)):
                bad = (h.backing[lo:hi] != self.sentinel).nonzero()
                if bad.numel():
                    found.append((h.entry, side, lo + int(bad[0]) - end, lo + int(bad[-1]) - end, h.asked))
        return found

    def check(self):
        found = self.violations()
        if found:
            raise GuardViolation("; ".join(
                f"{entry}: guard {side} the scratch changed, bytes {first:+d} .. {last:+d} relative to the body's end "
                f"({asked} bytes requested)" for entry, side, first, last, asked in found))

    def short_tails_intact(self):
        """short=k: the k withheld bytes of every body still hold the fill."""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return all(bool((h.backing[h.start + h.given:h.start + h.asked] == self.fill).all()) for h in self.handed)

    def shortened_bodies_intact(self):
        """short=k: every body that was handed out short -- the call that got it must have been refused before any launch --
        still holds the fill in all of its requested bytes; and there is at least one such body."""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        short = [h for h in self.handed if h.given < h.asked]
        return bool(short) and all(bool((h.backing[h.start:h.start + h.asked] == self.fill).all()) for h in short)
