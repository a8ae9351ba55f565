"""Forward reliability with function-valued posterior draws, on the device (paths.failure_probability,
emulator.failure_probability, gp.failure_probability; DESIGN I.22): with the inputs distributed over a box, how probable is
it that an output crosses a threshold, and how sure is the emulator of that probability?

Conditional on one draw f_p of the emulated function the failure probability is
    P_F(f_p) = prior{x : f_p(x) >= threshold},
and counting hits of a plain Monte-Carlo sample needs about 100 / P_F rows per draw.  Subset simulation (Au and Beck 2001; in
its sequential Monte-Carlo form Cerou, Del Moral, Furon and Guyader 2012) reaches the event through a ladder of levels of
conditional probability about level_prob each: R particles per draw from the prior; a stage takes the floor(level_prob R)-th
largest score as the next level, clones the particles at or above it (dgpamd_boxsus_level, one workgroup per draw) and moves
every clone n_moves times by the component-wise modified Metropolis step inside the level set (dgpamd_boxsus_move, one lane
per particle), until the level reaches the threshold.  P_F is the product of the stages' shares of survivors.  It needs no
gradient.  The spread of the P probabilities over the draws is the emulator's posterior uncertainty about P_F.
"""
import numpy as np
import torch

from . import optimize
from .ops import Engine
from .population import DeviceStageStreams, HostStreams, check_prior, check_rng, draw_status, particles, prior_particles, run_stages

STATUS = Engine.BOXSUS
MAX_PARTICLES = Engine.BOXSUS_MAXR
LAM_MIN, LAM_MAX = 1e-3, 1e2       # the clamp of a draw's step, in units of its survivors' spread


class SusStreams(HostStreams):
    """The random numbers of a subset-simulation run, children of np.random.SeedSequence(seed) by spawn key: (0, p) the prior
    uniforms of path p, (R, Dx); (1, p, t) and (2, p, t) the normal and the uniform draws of path p in stage t, (R, rounds,
    Dx) each, slot first.  A generator fills its array in index order, so slot r's numbers do not depend on R, and path p has
    generators of its own, so its numbers do not depend on P.  (rounds is one number per run: n_moves + 1.)"""

    def prior_uniforms(self):
        """(P, R, Dx) uniforms in [0, 1)."""
        return np.stack([self._rng(0, p).random((self.R, self.Dx)) for p in range(self.P)], 0)

    def stage(self, rounds):
        """(z (rounds, P, R, Dx), log u (rounds, P, R, Dx)) of the next stage."""
        t, self.t = self.t, self.t + 1
        z = np.stack([self._rng(1, p, t).standard_normal((self.R, rounds, self.Dx)) for p in range(self.P)], 0)
        with np.errstate(divide='ignore'):
            logu = np.log(np.stack([self._rng(2, p, t).random((self.R, rounds, self.Dx)) for p in range(self.P)], 0))
        return np.ascontiguousarray(z.transpose(2, 0, 1, 3)), np.ascontiguousarray(logu.transpose(2, 0, 1, 3))


class DeviceSusStreams(DeviceStageStreams):
    """SusStreams' twin for rng='device': population.DeviceStageStreams with Dx log u per particle and round and no resampling
    uniform; stage(rounds) gives (z (rounds, P, R, Dx), log u (rounds, P, R, Dx))."""

    def __init__(self, e, seed, P, R, Dx):
        super().__init__(e, seed, P, R, Dx, logu_elements=Dx, resample=False)


def n_survivors(level_prob, R):
    """n_s = max(1, floor(level_prob R)): the rank of the score that becomes the next level."""
    return max(1, int(np.floor(float(level_prob) * int(R))))


def prior_spread(x0):
    """(P, Dx): the spread per column of the prior particles x0 (P, R, Dx), the proposal's width before the first level."""
    return np.ascontiguousarray(np.std(x0, axis=1))


class FailureProbability:
    """The failure probabilities of P function-valued draws by subset simulation (failure_probability, DESIGN I.22).
    prob, log_prob (P,): the estimate of P_F(f_p) = prior{score >= 0}, score = +-(f_output - threshold).  levels, cond_prob,
    accept_rate, step (P, T) per stage: the level in score units (exactly 0 in a draw's final stage), the share of survivors
    n_b / R, the acceptance rate of the stage's moves and the step they used; NaN after a draw has finished.  x (P, R, Dx),
    score (P, R): for an ok draw R samples of prior(x | F) after the last stage's moves, and their scores.  status (P,):
    reliability.STATUS (= Engine.BOXSUS): ok 0; nan 1 no particle had a finite value (prob NaN); max_stages 2 the ladder
    ended below the threshold; below_min 3 the running product fell under min_prob.  For the last two prob estimates
    P(score >= the last level), which bounds P_F from above, and x samples that level set.  n_stages; evaluations: the walk
    evaluations of the stages, n_stages (n_moves + 1) -- the one of the prior particles comes on top.  rng: 'numpy' or 'device', where
    the run's random numbers were made.
    The spread of prob over the draws is the emulator's uncertainty about P_F; cov() is the Monte-Carlo error of one draw's
    number."""

    def __init__(self, prob, levels, cond_prob, accept_rate, step, x, score, status, n_stages, evaluations, rng='numpy'):
        self.rng = rng
        self.prob, self.levels, self.cond_prob, self.accept_rate, self.step = prob, levels, cond_prob, accept_rate, step
        self.x, self.score, self.status, self.n_stages, self.evaluations = x, score, status, n_stages, evaluations

    @property
    def log_prob(self):
        with np.errstate(divide='ignore'):
            return np.log(self.prob)

    def cov(self):
        """(P,): sqrt(sum_t (1 - c_t) / (c_t R)), c_t the stages' conditional probabilities: Au and Beck's coefficient of
        variation of prob with the correlation of the chains ignored (their gamma = 0).  The clones of one survivor are
        correlated, so this is a LOWER bound of the true coefficient of variation; the host test of DESIGN I.22 holds the
        spread over seeds to twice it."""
        R, c = self.x.shape[1], self.cond_prob
        with np.errstate(invalid='ignore', divide='ignore'):
            out = np.sqrt(np.nansum((1.0 - c) / (c * R), axis=1))
        return np.where(np.isnan(self.prob), np.nan, out)

    def summary(self, level=0.95):
        """Over the draws with a number: {'mean': the predictive failure probability E_f[P_F(f)], 'median', 'lower', 'upper':
        the equal-tailed interval of probability `level` of the per-draw probabilities -- the emulator's uncertainty --,
        'n_bounded': the draws whose prob is only an upper bound (status max_stages or below_min), 'mc_cov': the median of
        cov(), the Monte-Carlo error of one draw's number}."""
        if not 0.0 < level < 1.0:
            raise ValueError('summary: level must lie in (0, 1)')
        good = ~np.isnan(self.prob)
        if not good.any():
            raise ValueError('summary: no draw with a finite value')
        tail, pr = 0.5 * (1.0 - level), self.prob[good]
        return {'mean': float(pr.mean()), 'median': float(np.median(pr)), 'lower': float(np.quantile(pr, tail)),
                'upper': float(np.quantile(pr, 1.0 - tail)),
                'n_bounded': int(np.sum((self.status == STATUS['max_stages']) | (self.status == STATUS['below_min']))),
                'mc_cov': float(np.median(self.cov()[good]))}


def check_arguments(threshold, K, output, n_particles, level_prob, n_moves, max_stages, min_prob, step, target_accept):
    """failure_probability's refusals beside the bounds' and the prior's; (R, n_s, n_moves, max_stages, output)."""
    what = 'failure_probability'
    R, n_moves, max_stages, output = int(n_particles), int(n_moves), int(max_stages), int(output)
    if not np.isfinite(threshold):
        raise ValueError(what + ': threshold must be a finite number')
    if not 0 <= output < K:
        raise ValueError(what + ': output must lie in 0 .. %d' % (K - 1))
    if not 2 <= R <= MAX_PARTICLES:
        raise ValueError(what + ': need 2 <= n_particles <= %d' % MAX_PARTICLES)
    if not 0.0 < level_prob < 1.0 or np.floor(level_prob * R) >= R:
        raise ValueError(what + ': level_prob must lie in (0, 1) with floor(level_prob n_particles) < n_particles')
    if n_moves < 1 or max_stages < 1:
        raise ValueError(what + ': need n_moves >= 1 and max_stages >= 1')
    if not 0.0 <= min_prob < 1.0:
        raise ValueError(what + ': min_prob must lie in [0, 1)')
    if not (np.isfinite(step) and LAM_MIN <= step <= LAM_MAX) or not 0.0 < target_accept < 1.0:
        raise ValueError(what + ': need %g <= step <= %g and 0 < target_accept < 1' % (LAM_MIN, LAM_MAX))
    return R, n_survivors(level_prob, R), n_moves, max_stages, output


def failure_probability(e, P, K, Dx, values, threshold, bounds, output=0, below=False, n_particles=1024, level_prob=0.1,
                        n_moves=4, max_stages=50, min_prob=1e-12, seed=None, step=1.0, prior=None, target_accept=0.44,
                        rng='numpy'):
    """The driver behind PathFunctions.failure_probability and GpPaths.failure_probability.  values(xt (P, R, Dx)) -> (P, R, K):
    the walk at per-path rows, values only.  A stage of population.run_stages is dgpamd_boxsus_level, then n_moves + 1 walk
    evaluations with dgpamd_boxsus_move behind each: the start at the cloned particles, then n_moves decisions.  A draw's step
    lam is fixed within a stage and follows the stage's acceptance rate afterwards, on the device; the width itself is the
    survivors' spread, which the level step refreshes.  Only the count of unfinished draws visits the host, once per stage.
    rng='device': every random number is made on the device (DeviceSusStreams); the prior uniforms visit the host once, for
    prior_draws."""
    device_rng = check_rng(rng, 'failure_probability')
    lo, hi = optimize.check_bounds(bounds, Dx, 'failure_probability')
    Dx = len(lo)
    pv, pm = check_prior(prior, Dx)
    R, n_s, n_moves, max_stages, output = check_arguments(threshold, K, output, n_particles, level_prob, n_moves, max_stages,
                                                           min_prob, step, target_accept)
    sign = -1.0 if below else 1.0
    streams = DeviceSusStreams(e, seed, P, R, Dx) if device_rng else SusStreams(seed, P, R, Dx)
    x0 = prior_particles(streams, lo, hi, pv, pm)
    xt = e.tensor(x0)
    state = e.boxsus_state(P, R, Dx, lo, hi, pv, pm, step)
    state['sd'].copy_(e.tensor(prior_spread(x0)))
    active, levels, nsurv, lams = [], [], [], []

    move = lambda z, logu, first, last: e.boxsus_move(state, values(xt), xt, z, logu, threshold, output, sign, first=first, last=last)

    def level():
        active.append(state['done'] == 0)
        e.boxsus_level(state, xt, n_s, min_prob)
        levels.append(state['level'].clone()), nsurv.append(state['nsurv'].clone()), lams.append(state['lam'].clone())
    # the scores of the prior particles: a stage's start that ends at once (z and log u are not read)
    move(e.zeros(P, R, Dx), e.zeros(P, R, Dx), first=True, last=True)
    # the draw's step for the next stage follows this stage's acceptance over all its particles
    accept = run_stages(e, streams, state, n_moves, max_stages, target_accept, level, move,
                        lambda gain: state['lam'].mul_(gain).clamp_(LAM_MIN, LAM_MAX))
    host = {k: state[k].cpu().numpy() for k in ('x', 'score', 'prob', 'done', 'draw_status')}
    T = len(levels)
    on = torch.stack(active, 1).cpu().numpy()
    stack = lambda ts: np.where(on, torch.stack(ts, 1).double().cpu().numpy(), np.nan)
    return FailureProbability(host['prob'], stack(levels), stack(nsurv) / R, stack(accept), stack(lams), particles(host['x'], P, R),
                              host['score'].reshape(P, R), draw_status(STATUS, host['draw_status'], host['done'] == 0), T,
                              T * (n_moves + 1), rng)
