"""One byte buffer that holds every pointer argument of a call at exactly its documented size, with poison in between.

A kernel is tested for what it computes by the other tests; this helper is for WHERE it reads and writes.  Every buffer of a
call is placed in one allocation (the arena) at a 256-byte boundary, nbytes long and not a byte more, with at least GAP bytes
on either side that belong to no buffer.  fill(pattern) writes the pattern to all of those bytes (and the buffers' initial
contents into the buffers), the call runs, and
  * a WRITE outside a buffer shows as a gap byte that no longer holds the pattern: violations();
  * a READ outside a buffer shows as an output that differs between two fills, or from the ordinary call's: report().
A wrong kernel fails an assertion and cannot fault the card as long as what it touches stays inside the arena: the gaps are
sized for the cases (slack_rows for arrays that are indexed by a value the case controls).

The poison patterns have the top bit of every byte set.  Read as an int32 or int16 index they are negative — "none" everywhere
in this library, so a kernel never FOLLOWS a poison value —, as f32 they are NaN (0xFF) or a tiny negative number (0x80), and
as a flag byte they differ in both flag bits (SEARCHABLE = 1, OBSERVED = 2).

The backing is a numpy array (the helper's own test, with numpy stand-ins for kernels) or a torch.uint8 CUDA tensor.  No
fixtures, no pytest: a plain module."""
import numpy as np

POISONS = (0xFF, 0x80)
GAP = 4096
ALIGN = 256


def _up(x, a):
    return (x + a - 1) // a * a


class Arena:
    def __init__(self, device="numpy"):
        """device: "numpy" or "cuda" """
        self.device = device
        self._bufs = {}          # name -> (offset, nbytes, initial bytes (uint8 array))
        self._order = []
        self._end = GAP          # the first byte a new buffer may be placed at (the gap before it included)
        self._mem = None
        self._base = 0
        self.pattern = None

    # -- placing ---------------------------------------------------------------------------------------------------------
    def place(self, name, array_or_nbytes, slack_rows=0, row_bytes=0, init=0):
        """A buffer of exactly the array's bytes (its contents are the buffer's initial contents, restored by every fill), or
        of nbytes bytes that start as `init`.  slack_rows * row_bytes: the least gap behind it.  -> its offset"""
        if self._mem is not None:
            raise RuntimeError("the arena is laid out: place every buffer before the first fill")
        if name in self._bufs:
            raise KeyError("buffer %r placed twice" % name)
        if isinstance(array_or_nbytes, (int, np.integer)):
            data = np.full(int(array_or_nbytes), init, np.uint8)
        else:
            data = np.ascontiguousarray(array_or_nbytes).reshape(-1).view(np.uint8).copy()
        off = _up(self._end, ALIGN)
        self._bufs[name] = (off, len(data), data)
        self._order.append(name)
        self._end = off + len(data) + max(GAP, int(slack_rows) * int(row_bytes))
        return off

    def set_initial(self, name, array):
        """other initial contents of the same size for a placed buffer (the next fill writes them)"""
        off, n, _ = self._bufs[name]
        data = np.ascontiguousarray(array).reshape(-1).view(np.uint8).copy()
        if len(data) != n:
            raise ValueError("%r holds %d bytes, not %d" % (name, n, len(data)))
        self._bufs[name] = (off, n, data)

    @property
    def nbytes(self):
        return _up(self._end, ALIGN)

    def _allocate(self):
        total = self.nbytes + ALIGN
        if self.device == "numpy":
            self._mem = np.zeros(total, np.uint8)
            addr = self._mem.ctypes.data
        else:
            import torch
            self._mem = torch.zeros(total, dtype=torch.uint8, device=self.device)
            addr = self._mem.data_ptr()
        self._base = _up(addr, ALIGN) - addr
        self._addr = addr + self._base
        self._outside = np.ones(self.nbytes, bool)
        for off, n, _ in self._bufs.values():
            self._outside[off:off + n] = False

    # -- filling and checking --------------------------------------------------------------------------------------------
    def fill(self, pattern):
        """pattern into every byte outside the buffers, the initial contents into the buffers"""
        if self._mem is None:
            self._allocate()
        img = np.full(self.nbytes, pattern, np.uint8)
        for off, n, data in self._bufs.values():
            img[off:off + n] = data
        self._store(img)
        self.pattern = pattern

    def _store(self, img):
        if self.device == "numpy":
            self._mem[self._base:self._base + self.nbytes] = img
        else:
            import torch
            self._mem[self._base:self._base + self.nbytes].copy_(torch.from_numpy(img))
            torch.cuda.synchronize()

    def _load(self):
        if self.device == "numpy":
            return self._mem[self._base:self._base + self.nbytes].copy()
        import torch
        torch.cuda.synchronize()
        return self._mem[self._base:self._base + self.nbytes].cpu().numpy()

    def violations(self):
        """Every run of bytes outside the buffers that no longer holds the pattern -> list of dict(start, nbytes, buffer
        (the nearest), where ("behind" / "before"), distance (bytes from that buffer's end / start; 0 = adjacent), text)."""
        bad = np.flatnonzero(self._outside & (self._load() != self.pattern))
        if not len(bad):
            return []
        cuts = np.flatnonzero(np.diff(bad) > 1)
        starts, ends = bad[np.r_[0, cuts + 1]], bad[np.r_[cuts, len(bad) - 1]] + 1
        out = []
        for s, e in zip(starts.tolist(), ends.tolist()):
            best = None
            for name in self._order:
                off, n, _ = self._bufs[name]
                cand = ("behind", s - (off + n)) if s >= off + n else ("before", off - e)
                if best is None or cand[1] < best[2]:
                    best = (name, cand[0], cand[1])
            out.append(dict(start=s, nbytes=e - s, buffer=best[0], where=best[1], distance=best[2],
                            text="%d byte(s) written %d byte(s) %s %r" % (e - s, best[2], best[1], best[0])))
        return out

    # -- access ----------------------------------------------------------------------------------------------------------
    def offset(self, name):
        """the buffer's offset in mem (numpy stand-ins index mem as a kernel indexes memory)"""
        return self._base + self._bufs[name][0]

    @property
    def mem(self):
        return self._mem

    def ptr(self, name):
        if self._mem is None:
            self._allocate()
        return self._addr + self._bufs[name][0]

    def size(self, name):
        return self._bufs[name][1]

    def read(self, name, dtype=np.uint8):
        off, n, _ = self._bufs[name]
        if self.device == "numpy":
            raw = self._mem[self._base + off:self._base + off + n].copy()
        else:
            import torch
            torch.cuda.synchronize()
            raw = self._mem[self._base + off:self._base + off + n].cpu().numpy()
        return raw.view(dtype)


def report(arena, call, outputs, want=None, before_fill=None):
    """Run call(arena) once under each poison pattern (before_fill(arena, pattern), if given, first: set_initial of what is to
    hold the pattern inside a buffer) -> (list of findings, one text each; empty: the call kept to its
    buffers, dict name -> bytes of the outputs under the first pattern).  Findings: bytes written outside the buffers, outputs
    that differ between the two patterns, outputs that differ from `want` (dict name -> array, compared byte for byte: the
    ordinary call's)."""
    found, got = [], {}
    for p in POISONS:
        if before_fill is not None:
            before_fill(arena, p)
        arena.fill(p)
        call(arena)
        for v in arena.violations():
            found.append("poison 0x%02X: %s" % (p, v["text"]))
        got[p] = {name: arena.read(name) for name in outputs}
    a, b = got[POISONS[0]], got[POISONS[1]]
    for name in outputs:
        d = np.flatnonzero(a[name] != b[name])
        if len(d):
            found.append("%r depends on the poison: %d byte(s) differ between 0x%02X and 0x%02X, the first at %d"
                         % (name, len(d), POISONS[0], POISONS[1], d[0]))
        if want is not None:
            w = np.ascontiguousarray(want[name]).reshape(-1).view(np.uint8)
            for p in POISONS:
                g = got[p][name]
                if len(w) != len(g):
                    found.append("%r: %d bytes, the ordinary call's %d" % (name, len(g), len(w)))
                    break
                d = np.flatnonzero(g != w)
                if len(d):
                    found.append("poison 0x%02X: %r differs from the ordinary call in %d byte(s), the first at %d"
                                 % (p, name, len(d), d[0]))
    return found, a
