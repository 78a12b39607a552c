"""NumPy statement of the tracker's adaptive start sampling and masked resets (general_motion_retargeting_amd/csrc/gmr_tracker_adaptive.hip,
DESIGN.md section 6n), written independently of the kernels: the bins of a library, the base distribution, an Adapt, the draw from the
bins and the masked reset.  Bins, counts, ``ema``, clip ids, float32 clocks and draw counters are what the device must reproduce bit for
bit; ``prob`` and ``cdf`` are float64 sums whose order the device chooses for itself, so they are compared within a bound and the integer
decisions are checked on the device's own ``cdf`` (``AdaptiveTracker.bin_cdf`` may be replaced)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_mirror as tm  # noqa: E402

F = np.float32
MAX_BINS, MAX_K = 1 << 22, 16


def round_half_away(x):
    """llround of a non-negative float64"""
    w = np.floor(x)
    return int(w) + int(x - w >= 0.5)


class Bins:
    """The bins of a library (``seg [C + 1]`` frame offsets, ``fps [C]``) under ``bin_seconds``, in frames: clip c has bins of
    ``F_c = max(1, llround(bin_seconds fps_c))`` frames, ``ceil(T_c / F_c)`` of them; bin k covers frames ``[k F_c, min((k + 1) F_c,
    T_c))``.  ``base[b] = Wn_c frames(b) / T_c`` with ``Wn_c`` the clip weight over the sum of the weights of the clips that have frames
    (added in clip order; ones without weights)."""

    def __init__(self, seg, fps, bin_seconds, clip_weights=None):
        seg = [int(x) for x in seg]
        C = len(seg) - 1
        self.C = C
        self.F = np.array([max(1, round_half_away(float(bin_seconds) * float(fps[c]))) for c in range(C)], dtype=np.int64)
        T = np.array([seg[c + 1] - seg[c] for c in range(C)], dtype=np.int64)
        nb = -(-T // self.F)
        self.bin_start = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
        self.Bt = int(self.bin_start[-1])
        if not 1 <= self.Bt <= MAX_BINS:
            raise ValueError(f"{self.Bt} bins")
        w = np.ones(C) if clip_weights is None else np.asarray(clip_weights, dtype=np.float64)
        wsum = 0.0
        for c in range(C):
            if T[c] > 0:
                wsum = wsum + float(w[c])
        if not wsum > 0:
            raise ValueError("every clip that has frames has weight zero")
        self.clip = np.repeat(np.arange(C), nb)                                  # the clip of a bin
        k = np.arange(self.Bt) - self.bin_start[self.clip]
        self.first = k * self.F[self.clip]                                       # first frame of a bin, counted in its clip
        self.frames = np.minimum(self.first + self.F[self.clip], T[self.clip]) - self.first
        self.last = self.bin_start[self.clip + 1] - 1                             # the last bin of a bin's clip
        self.wn = w / wsum
        self.base = self.wn[self.clip] * self.frames.astype(np.float64) / T[self.clip].astype(np.float64)
        self.fps = np.asarray(fps, dtype=np.float64)

    def bin_of_frame(self, c, lo):
        """the bin of frame ``lo`` (counted from the first frame of clip ``c``): integers only"""
        nb = int(self.bin_start[c + 1] - self.bin_start[c])
        return int(self.bin_start[c]) + min(int(lo) // int(self.F[c]), nb - 1)


def gamma_powers(K, gamma):
    g, out = 1.0, []
    for _ in range(K):
        out.append(g)
        g = g * float(gamma)
    return out


def adapt(bins, ema, fail_now, alpha, uniform, K, gamma):
    """One Adapt in float64, every line one rounding per operation -> ``(ema, s, prob, cdf)``; the caller zeroes ``fail_now``"""
    if not (1 <= K <= MAX_K and 0.0 <= alpha <= 1.0 and 0.0 <= uniform <= 1.0 and 0.0 < gamma <= 1.0):
        raise ValueError("adaptive parameters out of range")
    ema = (1.0 - alpha) * ema + alpha * np.asarray(fail_now).astype(np.float64)
    b = np.arange(bins.Bt)
    s = np.zeros(bins.Bt)
    for u, g in enumerate(gamma_powers(K, gamma)):
        s = s + g * ema[np.minimum(b + u, bins.last)]
    s = np.where(bins.wn[bins.clip] == 0.0, 0.0, s)
    S = float(np.sum(s))
    prob = bins.base.copy() if S == 0.0 else (1.0 - uniform) * s / S + uniform * bins.base
    cdf = np.concatenate([[0.0], np.cumsum(prob)[:-1]])
    return ema, s, prob, cdf


def philox4x32_many(c0, c1, key):
    """Philox4x32-10 for counters ``(c0[i], c1[i], 0, 0)`` at once -> words 0 and 1 as uint64 arrays"""
    c0, c1 = np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m32, sh = np.uint64(tm.M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> sh) ^ c1 ^ k0) & m32, p1 & m32, ((p0 >> sh) ^ c3 ^ k1) & m32, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1


def bin_draws(bins, cdf, w0, w1):
    """the draw from the bins for Philox words ``w0, w1`` (arrays) -> ``(bin, clip, time f32)``"""
    x = np.asarray(w0, dtype=np.uint64).astype(np.float64) * 2.0 ** -32
    b = np.searchsorted(cdf, x, side="right") - 1                      # the largest b with cdf[b] <= x (cdf[0] = 0)
    u = (np.asarray(w1, dtype=np.uint64) >> np.uint64(8)).astype(F) * F(2.0 ** -24)
    c = bins.clip[b]
    time = ((bins.first[b].astype(np.float64) + u.astype(np.float64) * bins.frames[b].astype(np.float64)) / bins.fps[c]).astype(F)
    return b, c, time


class AdaptiveTracker(tm.Tracker):
    """``tracker_mirror.Tracker`` plus ``set_adaptive / adapt / reset_done`` and, on an adaptive tracker, the redraw of a finished clip
    from the bins.  ``reset`` and ``assign`` are the parent's."""

    def __init__(self, library, num_envs, dt, clip_weights=None, **kw):
        super().__init__(library, num_envs, dt, clip_weights=clip_weights, **kw)
        self.clip_w = None if clip_weights is None else np.asarray(clip_weights, dtype=np.float64)
        self.bins = self.params = self.bin_seconds = None

    # ---- configuration ------------------------------------------------------------------------------------------------------
    def set_adaptive(self, bin_seconds=1.0, alpha=0.1, uniform=0.3, lookahead=4, gamma=0.8):
        if bin_seconds is None or bin_seconds <= 0:
            self.bins = self.params = self.bin_seconds = None
            return
        gamma_powers(lookahead, gamma)
        if not (1 <= lookahead <= MAX_K and 0.0 <= alpha <= 1.0 and 0.0 <= uniform <= 1.0 and 0.0 < gamma <= 1.0):
            raise ValueError("adaptive parameters out of range")
        same = self.bins is not None and bin_seconds == self.bin_seconds
        self.params = (float(alpha), float(uniform), int(lookahead), float(gamma))
        if same:                    # new parameters for the Adapts to come; the history stays and no Adapt runs
            return
        self.bins, self.bin_seconds = Bins(self.lib.seg, self.lib.fps, bin_seconds, self.clip_w), bin_seconds
        self.fail_now = np.zeros(self.bins.Bt, dtype=np.uint32)
        self.ema = np.zeros(self.bins.Bt)
        self.adapt()

    def adapt(self):
        if self.bins is None:
            raise ValueError("adaptive sampling is not configured")
        self.ema, self.s, self.prob, self.bin_cdf = adapt(self.bins, self.ema, self.fail_now, *self.params)
        self.fail_now[:] = 0

    def adaptive_state(self):
        return {"bin_start": self.bins.bin_start.astype(np.int32), "fail_now": self.fail_now.copy(), "ema": self.ema.copy(),
                "prob": self.prob.copy(), "cdf": self.bin_cdf.copy(),
                "clip_prob": np.bincount(self.bins.clip, weights=self.prob, minlength=self.bins.C)}

    # ---- bins and draws -------------------------------------------------------------------------------------------------------
    def bin_of(self, e):
        """the bin of environment e's clock, -1 for a bad assignment"""
        c = int(self.clip[e])
        ok, lo, _, _ = self.lib.frames([c], [np.float64(self.time[e])], self.loop)
        if not ok[0]:
            return -1
        return self.bins.bin_of_frame(c, int(lo[0]) - int(self.lib.seg[c]))

    def draw_bin(self, e):
        """one draw for environment e from the bins -> (clip, time f32)"""
        w = tm.philox4x32((e, int(self.draws[e]), 0, 0), self.key)
        self.draws[e] += 1
        _, c, t = bin_draws(self.bins, self.bin_cdf, [w[0]], [w[1]])
        return int(c[0]), t[0]

    # ---- the masked reset -----------------------------------------------------------------------------------------------------
    def reset_done(self, done=None, failed=None, env_ids=None, resample=True, time_offset_range=(0.0, 0.0)):
        lo, hi = F(time_offset_range[0]), F(time_offset_range[1])
        if self.bins is not None and (not resample or lo != 0 or hi != 0):
            raise ValueError("an adaptive tracker draws clip and start from its bins")
        ids = np.arange(self.N) if env_ids is None else np.asarray(env_ids, dtype=np.int64).reshape(-1)
        which = np.arange(len(ids)) if done is None else np.nonzero(np.asarray(done).reshape(-1)[:len(ids)])[0]
        inside = (ids[which] >= 0) & (ids[which] < self.N)             # (the id of an entry that is not done is never looked at)
        ignored = int((~inside).sum())
        self.ignored += ignored
        which = which[inside]
        envs = ids[which]
        if self.bins is not None:                                      # every environment once: the order of the entries does not matter
            B = self.bins
            if failed is not None:
                fe = envs[np.asarray(failed).reshape(-1)[which] != 0]
                ok, lo_row, _, _ = self.lib.frames(self.clip[fe], self.time[fe].astype(np.float64), self.loop)
                c = self.clip[fe][ok].astype(np.int64)
                k = (lo_row[ok] - self.lib.seg[c]) // B.F[c]
                np.add.at(self.fail_now, B.bin_start[c] + np.minimum(k, B.bin_start[c + 1] - B.bin_start[c] - 1), 1)
            w0, w1 = philox4x32_many(envs, self.draws[envs], self.key)
            self.draws[envs] += 1
            _, c, t = bin_draws(B, self.bin_cdf, w0, w1)
            self.clip[envs], self.time[envs] = c, t
            self.length[envs] = ((self.lib.seg[c + 1] - self.lib.seg[c]).astype(np.float64) / self.lib.fps[c]).astype(F)
            return ignored
        for e in envs:
            clip, u = self.draw(e)
            if resample:
                self.clip[e], self.length[e] = clip, self.clip_length(clip)
            self.time[e] = lo + (hi - lo) * u
        return ignored

    # ---- the step: a finished clip restarts from the bins ------------------------------------------------------------------------
    def step(self, sim=None):
        if self.bins is None:
            return super().step(sim)
        before = self.draws.copy()
        out = super().step(sim)                 # (the parent has drawn "clip by weight, time 0" for the finished ones: taken back)
        for e in np.nonzero(out["finished"])[0]:
            self.draws[e] = before[e]
            self.clip[e], self.time[e] = self.draw_bin(e)
            self.length[e] = self.clip_length(int(self.clip[e]))
        return out
