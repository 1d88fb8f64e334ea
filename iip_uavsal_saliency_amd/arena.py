"""Liveness planner of the engine's activation arena: which recorded ops use which buffer, and offsets in ONE pool such that
two buffers share addresses only when they are never live together.  The engine drives it: `begin` a pass, `lop` += 1 for every
logical op, `lane` / `fork` / `join` for where the op is recorded, `touch` for what it reads and writes; after the sizing pass
`close` and `place` fix the layout and the engine hands over the pool it allocates (`buf`).  Nothing here touches a device."""

ARENA_ALIGN = 1024                                            # floats (4 KB): every arena buffer starts on a page


class _ArenaRef:
    """An activation's place in the arena: `numel` floats at `off`, live over the recorded ops [first, last]
    (positions on the main lane's timeline; a use on a side lane counts from that lane's fork to its join).  Stands where a
    tensor stood in `V.t`, so every view of the buffer shares it; `data_ptr()` refuses to hand out an address outside the
    live range while a plan is being recorded -- a recorder that forgot to declare a use fails there, at build time."""
    __slots__ = ("arena", "aid", "numel_", "off", "first", "last", "lkey", "lfirst", "llast", "pinned")

    def __init__(self, arena, aid, numel):
        self.arena, self.aid, self.numel_ = arena, aid, int(numel)
        self.pinned = False                   # outlives the call: a range of its own, never poisoned (Arena.pin)
        self.off, self.first, self.last = None, None, None
        # lkey: (lane, index of its fork) while every use so far was recorded on that lane between that fork and its join
        # (its launches are then ordered among themselves on one stream: [lfirst, llast] in recording order), else "mixed"
        self.lkey, self.lfirst, self.llast = None, None, None

    def numel(self):
        return self.numel_

    def end(self):
        """Last logical op that may touch the buffer (a buffer private to a side lane: in that lane's own order)."""
        return self.llast if isinstance(self.lkey, tuple) else self.last

    def data_ptr(self):
        a = self.arena
        if a.dry:
            return 0
        lo, hi = (self.lfirst, self.llast) if isinstance(self.lkey, tuple) else (self.first, self.last)
        if a.recording and not (lo <= a.lop <= hi):
            raise RuntimeError("arena: %r is addressed by op %d outside its live range [%d, %d] -- a recorder did not declare "
                               "this use (Arena.touch)" % (self.aid, a.lop, lo, hi))
        return a.buf.data_ptr() + 4 * self.off

    def tensor(self):
        return self.arena.buf[self.off:self.off + self.numel_]


def arena_conflict(a, b):
    """Are two buffers `(numel, first, last[, lane key, lane first, lane last])` ever live together?  [first, last] are positions
    on the main lane's timeline (a side-lane use counts from the fork to the join); two buffers used ONLY on the same side lane
    between the same fork and join are ordered by that lane's stream, so for them the recording-order ranges decide."""
    if a[2] < b[1] or b[2] < a[1]:
        return False
    if len(a) > 3 and len(b) > 3 and a[3] is not None and a[3] == b[3] and isinstance(a[3], tuple):
        return not (a[5] < b[4] or b[5] < a[4])
    return True


def plan_arena(bufs, align=ARENA_ALIGN):
    """Offsets for buffers `[(numel, first, last[, lane key, lane first, lane last]), ...]` such that two buffers that are ever
    live together (`arena_conflict`) never overlap: biggest first, each at the lowest aligned offset free of every already-placed
    buffer it conflicts with.  Returns (offsets, total floats, lower bound = the largest sum of sizes live at one main-lane position)."""
    order = sorted(range(len(bufs)), key=lambda i: (-bufs[i][0], bufs[i][1]))
    placed, offs = [], [0] * len(bufs)
    rnd = lambda n: (n + align - 1) // align * align
    for i in order:
        n, f, l = bufs[i][:3]
        busy = sorted((o, o + rnd(bufs[j][0])) for (o, j) in placed if arena_conflict(bufs[i], bufs[j]))
        at = 0
        for lo, hi in busy:
            if at + rnd(n) <= lo:
                break
            at = max(at, hi)
        offs[i] = at
        placed.append((at, i))
    total = max([o + rnd(bufs[j][0]) for (o, j) in placed], default=0)
    # lower bound: at a main-lane position, everything live there -- of the buffers that are private to one side lane only the
    # largest set that is live together in that lane's own order
    events = sorted(set(b[1] for b in bufs))
    bound = 0
    for t in events:
        live = [b for b in bufs if b[1] <= t <= b[2]]
        tot = sum(rnd(b[0]) for b in live if not (len(b) > 3 and isinstance(b[3], tuple)))
        lanes = {}
        for b in live:
            if len(b) > 3 and isinstance(b[3], tuple):
                lanes.setdefault(b[3], []).append(b)
        for grp in lanes.values():
            tot += max(sum(rnd(c[0]) for c in grp if c[4] <= u <= c[5]) for u in set(c[4] for c in grp))
        bound = max(bound, tot)
    return offs, total, bound


class Arena:
    def __init__(self):
        self.refs = {}                        # buffer id -> _ArenaRef, in declaration order
        self.buf = None                       # the pool (float32), allocated by the engine once `place` has sized it
        self.stats = {}
        self.recording = True                 # a plan is being built: addresses are checked against live ranges
        self.begin(dry=True)

    def begin(self, dry):
        """Start a pass over the plan: the sizing pass (`dry`: buffers are declared, uses grow live ranges, every address is
        0) or the recording pass (buffers are looked up, addresses are real)."""
        self.dry = dry
        self.lop = -1                         # logical op index (poison fills of the debug mode do not count)
        self.lane = 0
        self._lane_open, self._lane_refs, self._serial, self._poisoned = {}, {}, 0, set()

    def ref(self, aid, numel) -> _ArenaRef:
        if self.dry:
            if aid in self.refs:
                raise RuntimeError("arena: buffer %r declared twice" % (aid,))
            self.refs[aid] = _ArenaRef(self, aid, numel)
        r = self.refs.get(aid)
        if r is None or r.numel_ != int(numel):
            raise RuntimeError("arena: buffer %r of the recording pass was not (or differently) declared in the sizing pass" % (aid,))
        return r

    def scratch(self, kind, numel) -> _ArenaRef:
        """An anonymous buffer: the passes declare them in the same order, so a serial number names it."""
        self._serial += 1
        return self.ref((kind, self._serial), numel)

    def pin(self, r):
        """`r` outlives a call (sizing pass): what it holds after one run is read by later runs that do not write it again (the
        output of the prior nets while the caller's priors stay the same).  `place` gives it a range that no other buffer ever
        gets, whatever the live ranges say, and `due` never names it for a poison fill."""
        if not isinstance(r, _ArenaRef) or r.arena is not self:
            raise RuntimeError("arena: only a buffer of this arena can be pinned")
        r.pinned = True

    def touch(self, *vs):
        """Declare that the op being recorded reads or writes these views.  Sizing pass: grows the live range of their arena
        buffers -- on a side lane from the lane's fork (it may start right there) to, at its join, the join (it may still
        be running until then)."""
        if not self.dry:
            return
        for v in vs:
            r = getattr(v, "t", None) if v is not None else None
            if not isinstance(r, _ArenaRef):
                continue
            lo = hi = self.lop
            key = "main"
            if self.lane != 0:
                lo = self._lane_open.get(self.lane, lo)
                self._lane_refs.setdefault(self.lane, set()).add(r)
                key = (self.lane, self._lane_open.get(self.lane, -1))
            r.first = lo if r.first is None else min(r.first, lo)
            r.last = hi if r.last is None else max(r.last, hi)
            r.lkey = key if r.lkey in (None, key) else "mixed"
            r.lfirst = self.lop if r.lfirst is None else min(r.lfirst, self.lop)
            r.llast = self.lop if r.llast is None else max(r.llast, self.lop)

    def fork(self, lane):
        """The op just opened forks `lane` off the main lane."""
        self._lane_open.setdefault(lane, self.lop)

    def join(self, lane):
        """The op just opened joins `lane`: what ran on the lane may have been running until here."""
        for r in self._lane_refs.pop(lane, ()):
            r.last = max(r.last, self.lop)
        self._lane_open.pop(lane, None)

    def close(self, n_ops):
        """End of the sizing pass of a plan of `n_ops` ops (a lane the plan never joined: live to the end)."""
        for lane in list(self._lane_refs):
            for r in self._lane_refs.pop(lane):
                r.last = max(r.last, n_ops)
        self._lane_open = {}

    def place(self, n_ops, keep=()):
        """Fix every buffer's offset; `keep`: buffers that are read back after the run.  Returns the pool's size in floats."""
        refs = list(self.refs.values())
        for r in refs:
            if r.first is None:                      # declared, never used by an op: keep it addressable for the whole plan
                r.first, r.last, r.lkey, r.lfirst, r.llast = 0, n_ops, "mixed", 0, n_ops
        for r in keep:
            r.last, r.lkey = n_ops, "mixed"
        offs, total, bound = plan_arena([(r.numel_, r.first, r.last, r.lkey, r.lfirst, r.llast) for r in refs])
        for r, o in zip(refs, offs):
            r.off = o
        # a pinned buffer's range is its own: where other buffers share the range the planner gave it (by liveness they may),
        # it moves to a range of its own behind the pool; where nobody does -- the concatenated prior maps of the real plans --
        # it stays.  Everything else stays exactly where the planner put it: pinning changes no other address
        rnd = lambda n: (n + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN
        shared = total
        for r in refs:
            if r.pinned:
                r.last, r.lkey = n_ops, "mixed"          # (what it holds is still wanted after the plan's last op)
                if any(q is not r and q.off < r.off + rnd(r.numel_) and r.off < q.off + rnd(q.numel_) for q in refs):
                    r.off = total
                    total += rnd(r.numel_)
        self.stats = {"arena_mb": total * 4 / 1e6, "live_bound_mb": bound * 4 / 1e6,
                      "unshared_mb": sum(r.numel_ for r in refs) * 4 / 1e6, "buffers": len(refs),
                      "pinned_mb": sum(rnd(r.numel_) for r in refs if r.pinned) * 4 / 1e6,
                      "pinned_extra_mb": (total - shared) * 4 / 1e6}
        return total

    def layout(self):
        """[(buffer id, offset, floats, first op, last op, lane key, first / last op in recording order)] of the arena, by offset
        (`arena_conflict` takes `t[2:]`)."""
        return sorted(((r.aid, r.off, r.numel_, r.first, r.last, r.lkey, r.lfirst, r.llast) for r in self.refs.values()),
                      key=lambda t: (t[1], t[3]))

    def due(self, final=False):
        """Debug mode, recording pass: [(buffer, lane)] whose poison fill is due in front of the next op (`final`: behind the
        last one) -- every buffer once, when the op that ends its live range has been recorded; by offset.  A buffer private to
        a side lane is released in that lane's own order: its fill goes on that lane (while the lane is open: behind its last
        launch there, in front of whatever the lane runs next), everything else on the main lane."""
        due = [r for r in self.refs.values() if r not in self._poisoned and not r.pinned and (final or r.end() < self.lop + 1)]
        self._poisoned.update(due)
        # (still live at the end of the plan -- taps, the history the state is read from: no fill)
        return [(r, r.lkey[0] if isinstance(r.lkey, tuple) and self._lane_open.get(r.lkey[0]) == r.lkey[1] else 0)
                for r in sorted(due, key=lambda r_: r_.off) if not (final and r.end() >= self.lop)]
