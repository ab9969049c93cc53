"""A numpy float32 restatement of the dense Adam step (msha_adam_step) and of the lazy scheme
that replays missed steps (msha_adam_rows_replay): ``row_step`` bookkeeping, catch-up before
a read, gap replay inside the step, chunked flush -- and the constructive schedule the tests
of the replay share.  One arithmetic for both sides (fp32 values, fused multiply-adds through
float64), so "lazy after a flush == dense" is an exact statement about the scheme."""
import math

import numpy as np

F32 = np.float32


def schedule(n=193, steps=12, pairs=48):
    """``steps`` pair lists ``(src, dst)`` (int64, ``pairs`` each) over ``n`` rows, built
    without a seed: row 0 is in every step, row 1 in steps 1 and 12 only, row 2 in steps 3
    and 4 only, rows 150.. in none, the rest filled from a fixed permutation of 3..149."""
    assert n >= 193 and steps >= 12 and pairs >= 4
    perm = (np.arange(147) * 53) % 147 + 3  # gcd(53, 147) = 1: a permutation of 3..149
    out = []
    for s in range(1, steps + 1):
        ends = [0]
        if s in (1, 12):
            ends.append(1)
        if s in (3, 4):
            ends.append(2)
        k = 0
        while len(ends) < 2 * pairs:
            ends.append(int(perm[(37 * s + k) % 147]))
            k += 1
        e = np.asarray(ends, dtype=np.int64)
        out.append((e[:pairs].copy(), e[pairs:].copy()))
    return out


def rows_of(step_pairs):
    return np.unique(np.concatenate(step_pairs))


def schedule_facts(sched):
    """The four facts the schedule is built for, asserted on its own lists."""
    touched = [set(rows_of(sp).tolist()) for sp in sched]
    assert all(0 in t for t in touched)
    assert [s + 1 for s, t in enumerate(touched) if 1 in t] == [1, 12]
    assert [s + 1 for s, t in enumerate(touched) if 2 in t] == [3, 4]
    assert not any(r in t for t in touched for r in range(150, 193))
    return touched


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64)
            + np.asarray(c, np.float64)).astype(F32)


def scalars(lr, b1, b2, t):
    """adam_scalars: beta ** t by squaring in double; (step_size, bc2_sqrt) as fp32."""
    p1 = p2 = 1.0
    s1, s2, e = b1, b2, int(t)
    while e:
        if e & 1:
            p1 *= s1
            p2 *= s2
        s1 *= s1
        s2 *= s2
        e >>= 1
    return F32(lr / (1.0 - p1)), F32(math.sqrt(1.0 - p2))


def adam_elem(hp, t, g, p, m, v):
    """adam_elem on fp32 arrays: the new (p, m, v) of step t."""
    lr, b1, b2, eps, wd = hp
    step_size, bc2_sqrt = scalars(lr, b1, b2, t)
    g = _fma(F32(wd), p, g)
    m = _fma(F32(1.0 - b1), g - m, m)
    v = _fma(F32(1.0 - b2), g * g, v * F32(b2))
    denom = np.sqrt(v) / bc2_sqrt + F32(eps)
    return (p - step_size * (m / denom)).astype(F32), m, v


def dense_step(p, m, v, t, g, hp):
    """One dense step in place on (n, F) fp32 arrays; returns the new step count."""
    p[:], m[:], v[:] = adam_elem(hp, t + 1, g, p, m, v)
    return t + 1


class LazyTable:
    """The lazy scheme: ``row_step[r]`` is the step after which row r is valid."""

    def __init__(self, p):
        self.p = p.astype(F32).copy()
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.row_step = np.zeros(p.shape[0], np.int32)
        self.step = 0
        self.replayed = 0  # row-steps replayed (the shortcut's skipped ones excluded)

    def _replay(self, r, hp, max_steps):
        end = max(self.row_step[r], min(self.step, int(self.row_step[r]) + max_steps))
        p, m, v = self.p[r], self.m[r], self.v[r]
        zero = F32(0).tobytes()
        rest = (hp[4] == 0 and hp[3] > 0 and m.tobytes() == zero * m.size
                and v.tobytes() == zero * v.size and np.isfinite(p).all())
        if not rest:  # (permitted shortcut: m = v = +0 and no decay: nothing moves)
            for t in range(int(self.row_step[r]) + 1, int(end) + 1):
                p, m, v = adam_elem(hp, t, np.zeros_like(p), p, m, v)
                self.replayed += 1
        self.p[r], self.m[r], self.v[r] = p, m, v
        self.row_step[r] = end

    def catch_up(self, rows, hp, max_steps=2 ** 31 - 1):
        """Before a read of ``rows`` (distinct)."""
        for r in rows:
            self._replay(int(r), hp, max_steps)

    def step_rows(self, rows, g, hp):
        """One step: ``g[i]`` is the gradient of row ``rows[i]`` (distinct); any gap of a
        stepped row is replayed first."""
        for i, r in enumerate(rows):
            r = int(r)
            self._replay(r, hp, 2 ** 31 - 1)
            assert self.row_step[r] == self.step
            self.p[r], self.m[r], self.v[r] = adam_elem(hp, self.step + 1, g[i], self.p[r],
                                                        self.m[r], self.v[r])
            self.row_step[r] = self.step + 1
        self.step += 1

    def flush(self, hp, chunk):
        """ceil(T / chunk) passes over every row, at most ``chunk`` replayed steps each."""
        launches = -(-self.step // chunk)
        for _ in range(launches):
            self.catch_up(range(self.p.shape[0]), hp, chunk)
        return launches

    def stale_rows(self):
        return int((self.row_step < self.step).sum())
