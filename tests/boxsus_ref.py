"""dgpamd_boxsus_level and dgpamd_boxsus_move (csrc/boxsus.hip, DESIGN I.22) restated in numpy from the text of
include/dgp_amd.h, operation for operation on float64 numbers, so that the device's levels, survivors, ancestors, spreads,
trial points, decisions and counts can be compared with array_equal.  Also sus, the driver's schedule for one draw, and the
exact probabilities of the events the tests use.

The contract.  Draw p has R particles, lane q = p R + r.  score = sign (f_output - threshold) + 0.0 (the + 0.0 turns -0 into
+0), F = {score >= 0}.  A particle whose score is NaN is dead: never a survivor, the divisor stays R.
n_s = max(1, floor(level_prob R)).
LEVEL (a draw with done = 0): k = min(n_s, live count), b = the k-th largest live score; b >= 0: the level is +0.0 and the
stage is the draw's last; survivors = live particles with score >= level in increasing index, n_b of them;
prob *= (double)n_b / (double)R; done when the stage is final, or when prob < min_prob (status BELOW_MIN);
anc[j] = the (j mod n_b)-th survivor; sd_d = sqrt(sum_surv (x_d - mean_d)^2 / n_b) in the device's order (wg_sum), a value
that is 0 or not finite keeps the old one.  No live particle: status NAN, prob NaN, done.  done = 1: the identity.
MOVE: SCORE, INIT (first), DECIDE (first = 0, status OK: accept iff moved and score' >= level), HOLD (status NAN, or last),
PROPOSE (component-wise: c = x_d + (lam sd_d) z_d kept iff inside the box and, where pv_d > 0,
logu_d < ((-0.5 (pv_d e')) e') - ((-0.5 (pv_d e)) e)).
Step: lam <- clamp(lam exp(rate - target), 1e-3, 1e2) after every stage."""
import math

import numpy as np

OK, NAN, MAX_STAGES, BELOW_MIN = 0, 1, 2, 3
F = np.float64
LAM_MIN, LAM_MAX = 1e-3, 1e2
THREADS = 1024


# ------------------------------------------------------------------------------------------------------------------- LEVEL
def n_threads(R):
    return min(THREADS, (R + 63) // 64 * 64)


def wg_sum(v, mask):
    """The sum of v[mask] in the device's order, which R = len(v) alone fixes: thread t of T adds its particles t, t + T, ...
    in order, the 64 lanes of a wave combine by an xor butterfly 32, 16, .. 1, the wave totals add in index order."""
    R, T = len(v), n_threads(len(v))
    part = np.zeros(T)
    t = np.arange(T)
    for j in range((R + T - 1) // T):
        i = t + j * T
        idx = np.where(i < R, i, 0)
        add = (i < R) & mask[idx]
        part = np.where(add, part + v[idx], part)
    w = part.reshape(-1, 64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lanes ^ off]
    s = w[0, 0]
    for k in range(1, len(w)):
        s = s + w[k, 0]
    return s


def keys(score):
    """The order-preserving 64-bit keys of score + 0.0: all bits of a negative double flipped, the sign bit of a non-negative
    one; 0 for a NaN, which no number has."""
    s = np.asarray(score, dtype=F) + F(0.0)
    b = s.view(np.uint64)
    k = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(s), np.uint64(0), k)


def level(score, x, prob, sd, n_s, min_prob, done=False, status=OK):
    """One draw's LEVEL from score (R,), x (R, D), prob, sd (D,): dict(level, nsurv, prob, done, status, anc, sd, running,
    final); level and nsurv None where the call does not touch them."""
    score = np.asarray(score, dtype=F) + F(0.0)
    R, D = x.shape
    ident = dict(level=None, nsurv=None, prob=F(prob), done=True, status=status, anc=np.arange(R), sd=np.array(sd, dtype=F),
                 running=0, final=False)
    if done:
        return ident
    live = ~np.isnan(score)
    if not live.any():
        return dict(ident, prob=F(np.nan), status=NAN, nsurv=0)
    k = min(n_s, int(live.sum()))
    b = np.sort(score[live])[::-1][k - 1]
    final = bool(b >= 0.0)
    lev = F(0.0) if final else b
    surv = live & (score >= lev)
    idx = np.nonzero(surv)[0]
    nb = len(idx)
    prob = F(prob) * (F(nb) / F(R))
    below = (not final) and bool(prob < min_prob)
    new = np.array(sd, dtype=F)
    with np.errstate(all='ignore'):
        for d in range(D):
            mean = wg_sum(x[:, d], surv) / F(nb)
            e = x[:, d] - mean
            v = np.sqrt(wg_sum(e * e, surv) / F(nb))
            if v > 0.0 and np.isfinite(v):
                new[d] = v
    return dict(level=lev, nsurv=nb, prob=prob, done=final or below, status=BELOW_MIN if below else status,
                anc=idx[np.arange(R) % nb], sd=new, running=int(not (final or below)), final=final)


# -------------------------------------------------------------------------------------------------------------------- MOVE
class Particles:
    """Q = P R particles, one array entry each; every operation is elementwise over the particles and the loop over the
    columns runs in index order.  move(f (Q, K), z (Q, D), logu (Q, D), level (P,), lam (P,), sd (P, D)) is one call of the
    move kernel: f holds the values at self.trial; afterwards self.trial holds the next points to evaluate."""

    def __init__(self, x0, R, lo, hi, threshold, output=0, sign=1.0, pv=None, pm=None, whole=False):
        Q, D = np.shape(x0)
        self.whole = whole                  # (not the contract: the whole-vector walk, the second rejected design of I.22)
        self.R, self.lo, self.hi = R, np.asarray(lo, dtype=F), np.asarray(hi, dtype=F)
        self.pv = np.zeros(D) if pv is None else np.asarray(pv, dtype=F)
        self.pm = np.zeros(D) if pm is None else np.asarray(pm, dtype=F)
        self.threshold, self.output, self.sign = F(threshold), output, F(sign)
        self.trial = np.array(x0, dtype=F)
        self.x, self.score = self.trial.copy(), np.zeros(Q)
        self.moved = np.zeros(Q, dtype=bool)
        self.status = np.zeros(Q, dtype=np.int32)
        self.n_prop, self.n_acc = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32)

    def move(self, f, z, logu, level, lam, sd, first=False, last=False):
        with np.errstate(all='ignore'):
            self._move(np.asarray(f, dtype=F), np.asarray(z, dtype=F), np.asarray(logu, dtype=F),
                       np.atleast_1d(np.asarray(level, dtype=F)), np.atleast_1d(np.asarray(lam, dtype=F)),
                       np.atleast_2d(np.asarray(sd, dtype=F)), first, last)

    def _move(self, f, z, logu, level, lam, sd, first, last):
        Q, D = self.trial.shape
        p = np.arange(Q) // self.R
        xt = self.trial
        st = self.sign * (f[:, self.output] - self.threshold) + F(0.0)
        if first:
            self.x, self.score = xt.copy(), st
            self.n_prop, self.n_acc = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32)
            self.moved = np.zeros(Q, dtype=bool)
            live = ~np.isnan(st)
            self.status = np.where(live, OK, NAN).astype(np.int32)
        else:
            live = self.status == OK
            acc = live & self.moved & (st >= level[p])
            self.x, self.score = np.where(acc[:, None], xt, self.x), np.where(acc, st, self.score)
            self.n_prop = self.n_prop + live
            self.n_acc = self.n_acc + acc
        hold = ~live | last
        xp, any_kept, all_kept = self.x.copy(), np.zeros(Q, dtype=bool), np.ones(Q, dtype=bool)
        for d in range(D):
            s, x = sd[p, d], self.x[:, d]
            c = x + (lam[p] * s) * z[:, d]
            keep = ~((s == 0.0) | (self.lo[d] == self.hi[d])) & (c >= self.lo[d]) & (c <= self.hi[d])
            if self.pv[d] > 0.0:
                et, e = c - self.pm[d], x - self.pm[d]
                keep = keep & (logu[:, d] < (F(-0.5) * (self.pv[d] * et)) * et - (F(-0.5) * (self.pv[d] * e)) * e)
            xp[:, d] = np.where(keep, c, x)
            any_kept, all_kept = any_kept | keep, all_kept & keep
        if self.whole:
            xp, any_kept = np.where(all_kept[:, None], xp, self.x), all_kept
        self.trial = np.where(hold[:, None], self.x, xp)
        self.moved = np.where(hold, self.moved, any_kept)


def sus(fun, x0, lo, hi, threshold, streams, n_s, n_moves=4, max_stages=50, min_prob=1e-12, step=1.0, target_accept=0.44,
        pv=None, pm=None, sign=1.0, output=0, p=0, adapt='sd'):
    """failure_probability's schedule for draw p of the streams (a reliability.SusStreams whose prior uniforms made x0
    (R, D)), fun(x (R, D)) -> f (R, K): the evaluation of the prior particles, sd from their spread, then per stage LEVEL,
    the start of the stage and n_moves decisions with the draw's step held fixed, and after the stage the step times
    exp(rate - target_accept), clamped.  adapt='sd' is the contract; 'step-only' never refreshes sd and 'whole' moves all
    columns or none (the two rejected designs of DESIGN I.22).  Returns dict(prob, levels, cond_prob, accept_rate, step, x, score, status, cov, parts)."""
    R, D = x0.shape
    pt = Particles(x0, R, lo, hi, threshold, output, sign, pv, pm, whole=adapt == 'whole')
    sd = np.ascontiguousarray(np.std(x0[None], axis=1))[0]
    sd0 = sd.copy()
    lam, prob, lev = F(step), F(1.0), F(-np.inf)
    pt.move(fun(pt.trial), np.zeros((R, D)), np.zeros((R, D)), lev, lam, sd, first=True, last=True)
    levels, conds, rates, lams, status = [], [], [], [], MAX_STAGES
    for stage in range(max_stages):
        z, logu = streams.stage(n_moves + 1)
        t = level(pt.score, pt.x, prob, sd, n_s, min_prob)
        prob, sd = t['prob'], (sd0 if adapt == 'step-only' else t['sd'])
        if t['status'] == NAN:
            status = NAN
            break
        lev = t['level']
        levels.append(lev), conds.append(t['nsurv'] / R), lams.append(lam)
        pt.trial = pt.x[t['anc']].copy()
        for i in range(n_moves + 1):
            pt.move(fun(pt.trial), z[i, p], logu[i, p], lev, lam, sd, first=i == 0, last=i == n_moves)
        rates.append(pt.n_acc.sum() / max(pt.n_prop.sum(), 1))
        lam = F(min(max(lam * np.exp(F(rates[-1]) - F(target_accept)), LAM_MIN), LAM_MAX))
        if t['done']:
            status = t['status']
            break
    c = np.array(conds)
    return dict(prob=prob, levels=levels, cond_prob=conds, accept_rate=rates, step=lams, x=pt.x, score=pt.score, status=status,
                cov=float(np.sqrt(np.sum((1.0 - c) / (c * R)))) if len(c) else np.nan, parts=pt)


# ------------------------------------------------------------------------------------------------------------- exact answers
def corner_offset(D, prob):
    """a with a^D / D! = prob: the event sum x >= D - a under the uniform prior on [0, 1]^D has that probability (a <= 1)."""
    return (prob * math.factorial(D)) ** (1.0 / D)


def corner(D, prob):
    """(fun, threshold, exact probability) of the corner event."""
    a = corner_offset(D, prob)
    assert a <= 1.0
    return (lambda x: np.sum(x, 1)[:, None]), D - a, a ** D / math.factorial(D)


def phi(t):
    return 0.5 * math.erfc(-t / math.sqrt(2.0))


def halfspace(D, beta, width=5.0):
    """(fun, threshold, exact probability, prior (pv, pm), bounds (lo, hi)) of the event sum x / sqrt(D) >= beta under
    independent standard normals truncated at +-width: the probability of the untruncated event is Phi(-beta), and the
    truncation changes it by less than 2 D Phi(-width) in absolute terms on either side of the ratio."""
    return (lambda x: (np.sum(x, 1) / math.sqrt(D))[:, None]), beta, phi(-beta), (np.ones(D), np.zeros(D)), \
        (np.full(D, -width), np.full(D, width))


def grid_measure(f_on_grid, grid, threshold, sign=1.0):
    """The uniform measure of {x : sign (f(x) - threshold) >= 0} on [grid[0], grid[-1]] from the values on the increasing grid,
    f taken as piecewise linear: a cell with both ends inside counts whole, one that crosses by its share."""
    s = sign * (np.asarray(f_on_grid, dtype=F) - threshold)
    a, b, h = s[:-1], s[1:], np.diff(grid)
    with np.errstate(all='ignore'):
        part = np.where((a >= 0.0) & (b >= 0.0), 1.0, np.where((a < 0.0) & (b < 0.0), 0.0,
                        np.where(a >= 0.0, a / (a - b), b / (b - a))))
    return float(np.sum(part * h) / (grid[-1] - grid[0]))
