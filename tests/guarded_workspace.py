"""An exact-size, guarded stand-in for kernels._workspace (a plain helper module, like tests/rowops_reference.py).

kernels._workspace hands every wrapper one grow-only buffer of at least 1 MiB and the wrappers pass its numel() as
ws_bytes, so a size query that reports less than the launches carve up and write is invisible to the suite: the write
lands on the buffer's slack.  GuardedWorkspace has the signature of kernels._workspace and is installed with pytest's
monkeypatch fixture:

    gw = GuardedWorkspace(fill=0xFF)
    monkeypatch.setattr(K, "_workspace", gw)
    ... call wrappers ...
    assert gw.check() >= 1

For every request it makes a FRESH uint8 buffer of G + align_up(nbytes, 512) + G bytes (G = 1 MiB), fills all of it with
one byte and returns the view buf[G : G + nbytes]: numel() is exactly the requested size (so the entry is told exactly
what its size query asked for), the view's base keeps the allocator's 512-byte alignment, and the contents are not the
zeros of a fresh allocation nor the plausible leftovers of the previous call (fill 0xFF: integer counters read -1 and
floats NaN; 0xA5: garbage; 0x00: the friendly case).  `short=True` returns a view one byte SHORTER than requested (requests
of 0 bytes are left alone): an entry must refuse it before it launches anything.  A request of 0 bytes gets an empty view,
whose data_ptr() is null as for every empty torch tensor: an entry whose size query is 0 must not touch its workspace.

check() synchronises and asserts, for every buffer handed out, that every byte outside [G, G + nbytes) still holds the
fill.  G is a condition, not a measurement: it only has to absorb an overrun so that it is reported here instead of
landing in someone else's memory.  What this cannot see: READS past the end of the workspace (they change no byte), writes
further out than G, and writes of the fill byte itself (hence three fills).  Because every request is a fresh allocation,
nothing may capture a HIP graph under this allocator.
"""
import torch

G = 1 << 20
ALIGN = 512
FILLS = (0x00, 0xFF, 0xA5)


def align_up(n: int, a: int = ALIGN) -> int:
    return -(-int(n) // a) * a


class GuardedWorkspace:
    def __init__(self, fill: int = 0xFF, short: bool = False):
        if fill not in FILLS:
            raise ValueError(f"fill must be one of {[hex(f) for f in FILLS]}, got {fill!r}")
        self.fill = fill
        self.short = short
        self.requests = []   # (whole buffer, requested bytes, bytes of the returned view)

    def __call__(self, nbytes: int, device) -> torch.Tensor:
        nbytes = int(nbytes)
        if nbytes < 0:
            raise ValueError(f"workspace request of {nbytes} bytes")
        buf = torch.full((G + align_up(nbytes) + G,), self.fill, dtype=torch.uint8, device=device)
        given = nbytes - 1 if (self.short and nbytes > 0) else nbytes
        self.requests.append((buf, nbytes, given))
        return buf[G:G + given]

    def _first_dirty(self, region: torch.Tensor):
        bad = region != self.fill
        if not bool(bad.any()):
            return None
        return int(torch.nonzero(bad)[0])

    def dirty(self):
        """[(request index, requested bytes, offset of the first dirty byte RELATIVE TO THE WORKSPACE END, i.e. >= 0 behind
        the workspace and < -nbytes in front of it)] over all requests; synchronises device buffers."""
        out = []
        for i, (buf, nbytes, _given) in enumerate(self.requests):
            if buf.is_cuda:
                torch.cuda.synchronize(buf.device)
            back = self._first_dirty(buf[G + nbytes:])
            if back is not None:
                out.append((i, nbytes, back))
            front = self._first_dirty(buf[:G])
            if front is not None:
                out.append((i, nbytes, front - G - nbytes))
        return out

    def check(self) -> int:
        """Assert every guard byte of every request still holds the fill; returns the number of requests."""
        bad = self.dirty()
        assert not bad, "; ".join(
            f"request {i} of {nbytes} bytes: first dirty guard byte at workspace end {off:+d}"
            + (" (behind the workspace)" if off >= 0 else " (in front of the workspace)") for i, nbytes, off in bad) \
            + f" [fill 0x{self.fill:02X}]"
        return len(self.requests)

    def interior_untouched(self) -> bool:
        """True when every byte INSIDE every workspace still holds the fill (after a refused call: nothing ran)."""
        for buf, nbytes, _given in self.requests:
            if buf.is_cuda:
                torch.cuda.synchronize(buf.device)
            if self._first_dirty(buf[G:G + nbytes]) is not None:
                return False
        return True

    def views(self):
        """The views handed out, in request order."""
        return [buf[G:G + given] for buf, _nbytes, given in self.requests]
