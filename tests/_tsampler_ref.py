"""fp64 NumPy restatement of the loss-aware timestep sampler (Nichol & Dhariwal 2021, "Improved DDPM", section 3.3; improved-diffusion's
LossSecondMomentResampler in resample.py) as include/vdx.h states it under "Loss-aware timestep sampling".  There is no reference code for
it in the project this one is modelled on, so parity is UNPINNED in the sense of DESIGN.md section 9: this file is the yardstick.

Against improved-diffusion: the same state (the last H losses per level, oldest first, and a fill count), the same probabilities
(sqrt of the mean square, mixed with uniform_prob of the uniform distribution), the same weights 1 / (T p_t), uniform with weights 1 until
every level is full.  Different: the draw is an inverse-CDF draw from the project's Philox stream (theirs: np.random.choice), entries whose
loss is not finite or whose level is out of range are skipped, and an all-zero or overflowing history falls back to uniform p."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.philox_ref import philox4x32_10      # noqa: E402


class RefSampler:
    def __init__(self, T, H=10, eps=0.001):
        self.T, self.H, self.eps = int(T), int(H), float(eps)
        self.hist = np.zeros((self.T, self.H), dtype=np.float64)
        self.count = np.zeros(self.T, dtype=np.int32)

    def load_state(self, hist, count):
        self.hist = np.array(hist, dtype=np.float64).reshape(self.T, self.H).copy()
        self.count = np.array(count, dtype=np.int32).reshape(self.T).copy()

    @property
    def warm(self):
        return bool((self.count >= self.H).all())

    def probabilities(self):
        uni = np.full(self.T, 1.0 / self.T)
        if not self.warm:
            return uni
        s = np.zeros(self.T)
        with np.errstate(all='ignore'):
            for j in range(self.H):                              # (in index order, one rounding per operation)
                s = s + self.hist[:, j] * self.hist[:, j]
            w = np.sqrt(s / self.H)
            W = float(np.sum(w))
            if not np.isfinite(W) or W <= 0.0:
                return uni
            return (w / W) * (1.0 - self.eps) + self.eps * (1.0 / self.T)

    def uniforms(self, batch, key, draw=0):
        """u_b = (m + 0.5) 2^-53, m the 53 bits (r0 << 21) | (r1 >> 11) of Philox(counter (b, 0, draw), key)."""
        b = np.arange(batch, dtype=np.uint64)
        M = np.uint64(0xFFFFFFFF)
        r = philox4x32_10((b & M).astype(np.uint32), (b >> np.uint64(32)).astype(np.uint32), np.uint32(draw & 0xFFFFFFFF),
                          np.uint32((draw >> 32) & 0xFFFFFFFF), np.uint32(key & 0xFFFFFFFF), np.uint32((key >> 32) & 0xFFFFFFFF))
        m = (r[0].astype(np.uint64) << np.uint64(21)) | (r[1].astype(np.uint64) >> np.uint64(11))
        return (m.astype(np.float64) + 0.5) * 2.0 ** -53

    def prefix(self):
        return np.cumsum(self.probabilities())

    def draw(self, batch, key, draw=0, t=None):
        """(t int32 [batch], iw float64 [batch])."""
        p = self.probabilities()
        if t is not None:
            t = np.asarray(t, dtype=np.int64).reshape(batch)
        elif not self.warm:
            t = np.minimum(np.floor(self.uniforms(batch, key, draw) * self.T).astype(np.int64), self.T - 1)
        else:
            t = np.minimum(np.searchsorted(np.cumsum(p), self.uniforms(batch, key, draw), side='right'), self.T - 1)
        if not self.warm:
            return t.astype(np.int32), np.ones(batch)
        return t.astype(np.int32), 1.0 / (self.T * p[np.clip(t, 0, self.T - 1)])

    def update(self, entries):
        """entries [n, 2] = (t, loss), one after the other in index order."""
        for tv, l in np.asarray(entries, dtype=np.float64).reshape(-1, 2):
            if not np.isfinite(tv) or not np.isfinite(l) or tv < 0 or tv >= self.T:
                continue
            t = int(tv)
            if self.count[t] == self.H:
                self.hist[t, :-1] = self.hist[t, 1:].copy()
                self.hist[t, -1] = l
            else:
                self.hist[t, self.count[t]] = l
                self.count[t] += 1


def estimator_variances(p, f2_mean, f_mean):
    """Closed forms for one draw t ~ p of the estimator iw_t l_t of (1/T) sum_t E[l_t], with iw_t = 1 / (T p_t), given the per-level
    second moments f2_mean and means f_mean: Var = sum_t p_t iw_t^2 E[l_t^2] - (mean)^2."""
    T = len(p)
    mean = float(np.mean(f_mean))
    return float(np.sum(f2_mean / (T * T * p)) - mean * mean)
