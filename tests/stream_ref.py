"""numpy restatement of the stream separator (include/ams_stream.h), built on tests/stitch_ref.py.

The reference project has no counterpart of this feature: the tests compare libams_stream.so and ams_hip/stream.py with THIS module, and
this module with stitch_ref.chunks / search / tracks / overlap_add on the whole stream.  A plain helper module: no pytest hooks, no fixtures.

    Stream(S, L, H, infer)           one stream: push(x) -> [S, m], close() -> [S, m]; .N, .D, .rows (every chunk it cut), .trks
    split(rng, N, hi)                a random split of N samples into blocks of 0 .. hi samples
"""
import numpy as np

from tests import stitch_ref as ref


class Stream(object):
    """infer: mix [L] -> est [S, L] for ONE chunk (called in chunk order)."""

    def __init__(self, S, L, H, infer):
        assert 1 <= S and 2 <= L and (L + 1) // 2 <= H <= L - 1
        self.S, self.L, self.H, self.V, self.infer = S, L, H, L - H, infer
        self.N = self.D = 0
        self.pending = np.zeros(0, np.float32)
        self.tail = np.zeros((S, self.V), np.float32)
        self.trk = np.arange(S, dtype=np.int32)
        self.wh = ref.w_head(self.V)
        self.wt = (np.float32(1.0) - self.wh).astype(np.float32)
        self.rows, self.trks, self.closed = [], [], False

    def _absorb(self, row):
        """chunk c = D with the samples `row` [L] -> its H output samples [S, H]"""
        S, H, V = self.S, self.H, self.V
        e = np.asarray(self.infer(row), np.float32)
        assert e.shape == (S, self.L)
        self.rows.append(row)
        out = np.empty((S, H), np.float32)
        if self.D == 0:
            new = np.arange(S, dtype=np.int32)
            out[:] = e[:, :H]
        else:
            with np.errstate(invalid='ignore', over='ignore'):
                d = (self.tail[:, None, :].astype(np.float64) - e[None, :, :V].astype(np.float64))
                Q = (d * d).sum(axis=-1)
            rel = ref.search(Q[None])[0][0]
            new = rel[self.trk]
            with np.errstate(invalid='ignore'):
                a = (self.wt[None] * self.tail[self.trk]).astype(np.float32)
                b = (self.wh[None] * e[new, :V]).astype(np.float32)
                out[:, :V] = (a + b).astype(np.float32)
            out[:, V:] = e[new, V:H]
        self.tail, self.trk = e[:, H:].copy(), new
        self.trks.append(new.copy())
        self.D += 1
        return out

    def push(self, x):
        assert not self.closed
        x = np.asarray(x, np.float32).reshape(-1)
        self.N += x.shape[0]
        self.pending = np.concatenate([self.pending, x])
        outs = []
        while self.N >= self.D * self.H + self.L:                  # cut: one push may make several chunks ready, or none
            outs.append(self._absorb(self.pending[:self.L].copy()))
            self.pending = self.pending[self.H:]
        assert self.pending.shape[0] == self.N - self.D * self.H < self.L
        return np.concatenate(outs, axis=1) if outs else np.zeros((self.S, 0), np.float32)

    def close(self):
        assert not self.closed
        self.closed = True
        S, L, H, V, N = self.S, self.L, self.H, self.V, self.N
        if N == 0:
            return np.zeros((S, 0), np.float32)                    # no model pass
        done = self.D * H                                          # emitted so far
        if self.D == 0 or N > (self.D - 1) * H + L:
            row = np.zeros(L, np.float32)
            row[:self.pending.shape[0]] = self.pending
            out = np.concatenate([self._absorb(row), self.tail[self.trk]], axis=1)
        else:
            out = self.tail[self.trk][:, :V]
        return out[:, :N - done].copy()


def split(rng, N, hi):
    """Block sizes in 0 .. hi that add up to N."""
    sizes, left = [], N
    while left > 0:
        k = min(int(rng.randint(0, hi + 1)), left)
        sizes.append(k)
        left -= k
    return sizes
