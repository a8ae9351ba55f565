"""Function-valued posterior draws of GP nodes by pathwise conditioning (emulator.sample_functions, gp.sample_functions;
DESIGN I.12).

A node with training inputs W (n, D), outputs y, replicate weights omega, R = c(W, W) + nugget diag(omega) = L L^T has the
prior draw  g(x) = phi(x)^T theta,  phi(x) = sqrt(2/F) cos(Omega x + b),  of F random Fourier features (features()), and
Matheron's rule turns it into a posterior draw:
    f(x) = sqrt(scale) (phi(x)^T theta + c(x, W) v),   v = L^-T L^-1 (y / sqrt(scale) - Phi(W) theta - sqrt(nugget omega) * eps),
theta ~ N(0, I_F), eps ~ N(0, I_n).  Its mean over (theta, eps) is c(x, W) R^-1 y for every F; its covariance tends to the
posterior's as F grows.  A path is held as (theta, v) and evaluated by dgpamd_pathfun_eval at any rows, any number of times,
with the same values at the same rows.

NodePaths is the paths of one node: draw_node alone consumes the generator at creation, and NodePaths.build_shared /
build_per_group condition its draws on a training side in the form paths.Dense.draw_shared / draw_per_path take theirs.
PathFunctions (an emulator: pathwalk.walk over its hierarchy, beside the drawers paths.Dense and vpaths.Vecchia) and GpPaths
(one node, numpy's global generator) are built from these and evaluate in blocks of rows through one loop, _row_blocks.
They hold node paths by interface (__call__, value_and_grad, noise_sd, Omega, m): vpathfun.VecchiaNodePaths, the update by
local conditioning of sample_functions_vecchia (DESIGN I.14), is built from the same draws and evaluated by the same code.

The input gradient of a path is as closed-form as the path (DESIGN I.13): dgpamd_pathfun_grad returns a node's values and
its (P, M, D) gradient from one pass, and PathFunctions.value_and_grad carries the Jacobian with respect to the emulator's
input through the same walk by the chain rule, on the device.

paths.sobol(A, B) (DESIGN I.16) evaluates the draws at a Saltelli design through the same walk, PathFunctions._walk, which
leaves every layer on the device, and takes the pick-freeze sums of their Sobol' indices there (sensitivity.pick_freeze).

paths.minimize(bounds) (DESIGN I.17) finds every draw's optimum over a box: the same walk at per-path rows (P, R, Dx), values
and Jacobian, feeds a batched projected L-BFGS on the device (optimize.minimize, dgpamd_boxmin_step).

paths.active_subspace(X) (DESIGN I.18) contracts the same walk's Jacobian at the rows of a design into every draw's
E_x[grad f grad f^T] on the device (sensitivity.gradient_moments, dgpamd_gradmom_tiles): the Jacobian never visits the host.

paths.calibrate(y, obs_sd, bounds) (DESIGN I.19) samples every draw's posterior of the input given an observation: the walk at
per-path rows feeds batched MALA or HMC chains on the device (calibrate.calibrate, dgpamd_boxmala_step, dgpamd_boxhmc_step).
paths.calibrate_smc (DESIGN I.21) feeds the same walk to tempered SMC particles, which also give every draw's evidence
(calibrate.calibrate_smc, dgpamd_boxsmc_temper, dgpamd_boxsmc_move).
paths.failure_probability (DESIGN I.22) feeds its values to subset-simulation particles: the probability of a rare event of
every draw (reliability.failure_probability, dgpamd_boxsus_level, dgpamd_boxsus_move).
"""
import copy

import numpy as np
import torch

from . import paths, pathwalk


def features(rng, kind, length, D, F):
    """(Omega (F, D), b (F,)) of a node's random Fourier features, drawn from rng (a numpy Generator, or the numpy.random
    module) in the order: standard_normal((F, D)); for 'matern2.5' chisquare(5, (F, D)); uniform(0, 2 pi, F).
    sexp: exp(-tau^2 / g^2) has spectral measure N(0, 2 / g^2): Omega = sqrt(2) z / g.  matern2.5 (the separable product):
    every column a Student-t with 5 degrees of freedom over g, Omega = z / sqrt(chi2_5 / 5) / g, independent per (f, d).
    One lengthscale is broadcast over the D columns."""
    g = np.broadcast_to(np.asarray(length, dtype=np.float64).reshape(-1), (D,)) if np.size(length) == 1 else \
        np.asarray(length, dtype=np.float64).reshape(D)
    z = rng.standard_normal((F, D))
    if kind == 'sexp':
        Omega = np.sqrt(2.0) * z / g
    elif kind == 'matern2.5':
        Omega = z / np.sqrt(rng.chisquare(5, (F, D)) / 5.0) / g
    else:
        raise ValueError(kind)
    b = rng.uniform(0.0, 2.0 * np.pi, F)
    return Omega, b


def _rows_per_call(e, P, width):
    """Rows evaluated per call: `width` doubles per row and path within a quarter of the free device memory."""
    free = torch.cuda.mem_get_info(e.device)[0]
    return int(max(1, free // 4 // (8 * P * width)))


def weights(e, hyper, W, Linv, Omega, b, theta, y, eps, omega):
    """v (P, n) of P paths that share one training set: W (n, D), Linv = paths.factor_inverse's L^-1, theta (P, F), y (P, n)
    or (n,), eps (P, n) device tensors, omega (n,) device tensor or None.  Phi(W) theta is the prior part of the paths at
    x = W (dgpamd_pathfun_eval with n = 0); L^-1 is applied by dgpamd_trmv_lower to 64 paths at a time, L^-T by dgpamd_gemv
    on the transposed triangle; one refinement step against R v follows."""
    kind, length, scale, nugget = hyper
    n = W.shape[0]
    P = theta.shape[0]
    LT = torch.tril(Linv[:n, :n]).T.contiguous()
    diag = nugget if omega is None else nugget * omega

    def solve(rhs):
        u, out = e.empty(P, n), e.empty(P, n)
        for p0 in range(0, P, 64):
            p1 = min(P, p0 + 64)
            e.trmv_lower(n, Linv, [1.0], rhs[p0:p1], batch=p1 - p0, out=u[p0:p1], shared=True)
        for p in range(P):
            e.gemv(LT, u[p], out=out[p])
        return out

    r = y / np.sqrt(scale) - e.pathfun_eval(kind, W, None, Omega, b, theta, None, length, 1.0)
    r -= eps * (np.sqrt(nugget) if omega is None else torch.sqrt(nugget * omega))
    r = r.contiguous()
    v = solve(r)
    # one step of iterative refinement: the explicit L^-1 leaves a residual of order cond(L) eps |R| |v|, and v is large where
    # R is ill-conditioned (a small nugget); R v = c(W, W) v + nugget omega * v is the evaluation kernel itself at x = W
    zero = e.zeros(1, W.shape[1])
    Rv = e.pathfun_eval(kind, W, W, zero, e.zeros(1), e.zeros(P, 1), v, length, 1.0) + diag * v
    return v + solve((r - Rv).contiguous())


def draw_node(rng, kind, length, D, F, S, J, n):
    """What is random in the S * J paths of one GP node, host arrays Omega (F, D), b (F,), theta (S * J, F), eps (S * J, n), in
    the order features(rng, kind, length, D, F), standard_normal((S, J, F)), standard_normal((S, J, n)); rng a numpy Generator
    or the numpy.random module.  S = 1 takes from the stream what (J, F) and (J, n) take.  An iterator: each array is drawn
    when it is asked for and not kept here, so list(map(e.tensor, draw_node(...))) holds one host array at a time."""
    yield from features(rng, kind, length, D, F)
    yield rng.standard_normal((S, J, F)).reshape(S * J, F)
    yield rng.standard_normal((S, J, n)).reshape(S * J, n)


class NodePaths:
    """P function-valued draws of one GP node: hyper = paths.hyper(node); Omega (F, D), b (F,) its features; theta (P, F);
    W (n, D) one training set for every path, or (G, n, D) with group (host ints (P,)) picking each path's; v (P, n).
    All its own copies.  build_*: train = (W, paths.factor_inverse's L^-1), omega (n,) or None, draws = draw_node's, all on the device."""

    m = 0   # neighbours looked up per row (vpathfun.VecchiaNodePaths: its conditioning-set size; _rows_per_call's width counts them)

    def __init__(self, hyper, Omega, b, theta, W, v, group=None):
        kind, length, scale, nugget = hyper
        self.hyper = (kind, np.array(length, dtype=np.float64), float(scale), float(nugget))
        self.Omega, self.b, self.theta, self.W, self.v = Omega, b, theta, W, v
        self.group = None if group is None else np.asarray(group, dtype=np.int32).copy()

    @classmethod
    def build_shared(cls, e, hyper, train, Y, omega, draws, rep):
        """One training set for every path, rows Y (R, n) of right-hand sides: path q of the R * rep is conditioned on row
        q // rep.  One weights call for all of them."""
        Om, b, theta, eps = draws
        W = train[0].clone()
        return cls(hyper, Om, b, theta, W, weights(e, hyper, W, train[1], Om, b, theta, Y.repeat_interleave(rep, 0), eps, omega))

    @classmethod
    def build_per_group(cls, e, hyper, train, y, omega, draws, group):
        """Every group its own training set: train[g] = (W, Linv), y[g] (n,) (lists, or paths.PerGroup); group host ints (P,),
        the paths of group 0, then those of group 1, ... (np.repeat(np.arange(G), J)).  One weights call per group."""
        Om, b, theta, eps = draws
        ends = np.searchsorted(group, np.arange(group[-1] + 2))   # (group g's paths: ends[g] .. ends[g + 1] - 1)
        Ws, vs = [], []
        for g in range(len(ends) - 1):
            (W, Linv), mine = train[g], slice(ends[g], ends[g + 1])
            Ws.append(W)
            vs.append(weights(e, hyper, W, Linv, Om, b, theta[mine], y[g], eps[mine], omega))
        return cls(hyper, Om, b, theta, torch.stack(Ws), torch.cat(vs), group)

    def _train(self, x):
        """(W, group) as the device entries take them with x: (M, D) shared by every path, or (P, M, D)."""
        if x.dim() == 3 and self.W.dim() == 2:
            return self.W[None], None
        return self.W, (self.group if x.dim() == 3 else None)

    def __call__(self, e, x):
        """The paths at x: (M, D) shared by every path, or (P, M, D).  Returns (P, M)."""
        kind, length, scale, _ = self.hyper
        W, group = self._train(x)
        return e.pathfun_eval(kind, x, W, self.Omega, self.b, self.theta, self.v, length, scale, group=group)

    def value_and_grad(self, e, x):
        """The paths and their input gradients at x ((M, D) shared, or (P, M, D)): (P, M), bit for bit what __call__
        returns, and (P, M, D), d path p at row m / d column d of its own input."""
        kind, length, scale, _ = self.hyper
        W, group = self._train(x)
        return e.pathfun_grad(kind, x, W, self.Omega, self.b, self.theta, self.v, length, scale, group=group)

    def noise_sd(self):
        return np.sqrt(self.hyper[2] * self.hyper[3])


def build_nodes(emu, sample_size, n_features, node):
    """{(l, k): node(l, k, nd, draw)} over the emulator's GP nodes in walk order (layer by layer, node by node).  draw(D)
    takes the node's draws from the emulator's sampling generator -- draw_node for D input columns and N * sample_size
    paths, on the device -- and is the only thing that consumes it: every kind of node paths built from equal generator
    states holds the same features, theta and eps."""
    e, rng = emu.engine, emu._sample_rng
    S, J, F = emu.N, int(sample_size), int(n_features)
    if J < 1 or F < 1:
        raise ValueError('sample_functions needs sample_size >= 1 and n_features >= 1')
    nodes = {}
    for l, layer in enumerate(emu.all_layer):
        for k, nd in enumerate(layer):
            if nd.type == 'gp':
                nodes[l, k] = node(l, k, nd, lambda D, nd=nd: list(map(e.tensor, draw_node(rng, nd.name, nd.length, D, F, S, J, len(nd.output)))))
    return nodes


def dense_nodes(emu, sample_size, n_features):
    """The NodePaths of a dense emulator, on its joint statistics (emu._joint_stats: L^-1 of every node and imputation)."""
    e, S, J = emu.engine, emu.N, int(sample_size)

    def node(l, k, nd, draw):
        hyper, st = paths.hyper(nd), emu._joint_stats(l, k)
        draws = draw((st['W'] if l == 0 else st['per'][0]['W']).shape[1])
        omega = None if nd.rep is None else e.tensor(nd.W_diag)
        if l == 0:
            return NodePaths.build_shared(e, hyper, (st['W'], st['Linv']), st['Y'], omega, draws, J)
        train = paths.PerGroup(lambda s: (st['per'][s]['W'], st['per'][s]['Linv']))
        return NodePaths.build_per_group(e, hyper, train, paths.PerGroup(lambda s: st['per'][s]['y']), omega, draws,
                                         np.repeat(np.arange(S), J))
    return build_nodes(emu, J, n_features, node)


def _row_blocks(e, x, P, width, multiple=1):
    """(m0, x[m0:m0 + step]) over the rows of x in order, contiguous blocks of step = _rows_per_call(e, P, width) rows,
    rounded down to a multiple of `multiple` and at least that (sensitivity.pick_freeze: its blocks start at tiles of 64)."""
    if len(x) == 0:
        raise ValueError('sample_functions: x has no rows')
    step = _rows_per_call(e, P, width)
    if multiple > 1:
        step = max(multiple, step // multiple * multiple)
    for m0 in range(0, len(x), step):
        yield m0, np.ascontiguousarray(x[m0:m0 + step])


def _join(blocks):
    """Per-block lists over layers of (P, rows, ...) arrays -> one list over layers, the blocks' rows in order."""
    return [np.concatenate(bl, 1) for bl in zip(*blocks)]


def _scatter_add(J, g, columns):
    """J[..., columns[i]] += g[..., i], column by column in the order given: a column named twice receives both terms, in a
    fixed order."""
    for i, c in enumerate(columns):
        J[..., int(c)] += g[..., i]


def check_pick_freeze(layers):
    """What sobol refuses: pick-freeze compares one function at rows that share some of their columns."""
    for layer in layers:
        for nd in layer:
            if nd.type != 'gp':
                raise ValueError('sobol: the draws of this emulator pass through a sampled node (a likelihood node or a '
                                 'Categorical top); a sampled node is drawn afresh on every evaluation, so a draw is not one '
                                 'function of x and the pick-freeze estimators of its Sobol\' indices mean nothing')


def _check_smooth(nodes, what='minimize', why='a gradient method has nothing to follow'):
    """What minimize and active_subspace refuse beside value_and_grad's own refusals, before they evaluate anything."""
    if any(nf.m for nf in nodes):
        raise NotImplementedError('%s: a draw made by local conditioning (sample_functions_vecchia) is only piecewise '
                                  'differentiable, so %s; sample_functions gives '
                                  'differentiable draws of a dense model' % (what, why))


class PathFunctions:
    """emulator.sample_functions' result: N * sample_size posterior draws of the emulated function, each a closed-form
    function of x.  paths(x, full_layer=False, noise=False) evaluates all of them at the rows of x and returns
    sample_paths' container: a list over the final layer's nodes of (M, N * sample_size) arrays, or with full_layer a list
    over layers of such lists; column s * sample_size + j is path j of imputation s.  Any number of rows (evaluated in
    blocks that fit the free device memory); GP nodes give the same values at the same rows in every call.  Drawn afresh
    on each call, block of rows by block of rows: the samples of likelihood nodes and of a Categorical top (from the path's
    latents by the node's own sampling(), which draws from numpy's global generator, as in sample_paths), and with
    noise=True an independent N(0, scale * nugget) term per row, path and GP node in walk order, from the emulator's
    sampling generator (standard_normal((N * sample_size, rows)) each) -- the
    nugget that sample_paths' joint covariance carries on its diagonal.  The object holds its own copies of the features,
    weights and training inputs: it stays valid when the emulator changes.
    paths.value_and_grad(x, full_layer=False) -> (values, gradients) and paths.grad(x, full_layer=False) -> gradients
    differentiate every draw with respect to the rows of x (emulators of GP nodes only): values is paths(x)'s container
    with paths(x)'s bits; gradients is a list over the final layer's nodes of (M, Dx, N * sample_size) arrays, Dx =
    x.shape[1], entry [m, d, s * sample_size + j] = d path / d x[m, d] (columns of x the model does not read: zero), or
    with full_layer a list over layers of such lists."""

    def __init__(self, emu, sample_size, n_features, nodes=None, after=None):
        """nodes: the (layer, node) -> node paths mapping of the emulator's GP nodes (build_nodes'; None: dense_nodes, what
        sample_functions returns); after(engine, node paths): called at the end of every paths(x) (vpathfun.check_status)."""
        self.nodes = dense_nodes(emu, sample_size, n_features) if nodes is None else nodes
        self.engine, self.rng, self.N, self.sample_size, self.n_features = emu.engine, emu._sample_rng, emu.N, int(sample_size), int(n_features)
        self.layers = [[copy.copy(nd) for nd in layer] for layer in emu.all_layer]
        self.after = after

    def __call__(self, x, full_layer=False, noise=False):
        paths.check_2d(x)
        e, P = self.engine, self.N * self.sample_size
        width = 4 * max(len(layer) for layer in self.layers) + 3 * max(nf.Omega.shape[1] for nf in self.nodes.values()) + 4 + \
            max(nf.m for nf in self.nodes.values())
        out = _join(self._block(xb, noise=noise)[0] for _, xb in _row_blocks(e, x, P, width))
        if self.after is not None:
            self.after(e, self.nodes.values())
        out = [list(a.transpose(2, 1, 0)) for a in out]
        return out if full_layer else out[-1]

    def _check_differentiable(self):
        for layer in self.layers:
            for nd in layer:
                if nd.type != 'gp':
                    raise ValueError('sample_functions: the draws of this emulator pass through a sampled node (a likelihood '
                                     'node or a Categorical top), and a sampled node has no derivative with respect to x; '
                                     'grad and value_and_grad need an emulator of GP nodes only (paths(x) still evaluates)')

    def value_and_grad(self, x, full_layer=False):
        """(values, gradients) at the rows of x (M, Dx).  values: paths(x, full_layer)'s container and bits.  gradients: a
        list over the final layer's nodes of (M, Dx, N * sample_size) arrays, [m, d, s * sample_size + j] = d (path j of
        imputation s at row m) / d x[m, d]; with full_layer a list over layers of such lists.  Columns of x that the model
        does not read get zero.  Raises ValueError for an emulator with a likelihood node or a Categorical top."""
        self._check_differentiable()
        paths.check_2d(x)
        e, P, Dx = self.engine, self.N * self.sample_size, x.shape[1]
        K, D = max(len(layer) for layer in self.layers), max(nf.Omega.shape[1] for nf in self.nodes.values())
        # paths(x)'s doubles per row and path, a node's gradient twice (the kernel's and the slice multiplied), and Dx per node
        # for the Jacobians of two layers, one gathered operand and the node's own
        width = 4 * K + 3 * D + 4 + 2 * D + (3 * K + 2) * Dx
        blocks = [self._block(xb, jacobians='all' if full_layer else 'last') for _, xb in _row_blocks(e, x, P, width)]
        vals = [list(a.transpose(2, 1, 0)) for a in _join(v for v, _ in blocks)]
        grads = [list(a.transpose(2, 1, 3, 0)) for a in _join(g for _, g in blocks)]
        return (vals, grads) if full_layer else (vals[-1], grads[-1])

    def grad(self, x, full_layer=False):
        """value_and_grad(x, full_layer)[1]."""
        return self.value_and_grad(x, full_layer)[1]

    def sobol(self, A, B):
        """Sobol' indices of every draw from the base samples A, B (n_base, Dx), host arrays of one shape, n_base >= 2
        (sensitivity.saltelli_design makes them): a sensitivity.SobolResult with first and total (K, Dx, N * sample_size),
        K the outputs of the last layer.  The draws are evaluated at A, B and the Dx designs AB_i in blocks of rows and
        summed on the device; the result does not depend on the blocks by a bit.  Raises ValueError for an emulator with a
        likelihood node or a Categorical top."""
        from . import sensitivity
        check_pick_freeze(self.layers)
        sensitivity.check_design(A, B)
        e, P = self.engine, self.N * self.sample_size
        # paths(x)'s doubles per row and path, and the three designs and three sets of values of a block
        width = 4 * max(len(layer) for layer in self.layers) + 3 * max(nf.Omega.shape[1] for nf in self.nodes.values()) + 4 + \
            max(nf.m for nf in self.nodes.values()) + 3 * len(self.layers[-1]) + 3 * A.shape[1]

        def evaluate(xd):
            for cur, _ in self._walk(xd):
                pass
            return cur
        sums = sensitivity.pick_freeze(e, evaluate, A, B, P, width)
        if self.after is not None:
            self.after(e, self.nodes.values())
        return sensitivity.SobolResult(sums, len(A))

    def minimize(self, bounds, n_starts=8, n_candidates=2048, output=0, maximize=False, x0=None, seed=None, qmc=False,
                 maxiter=100, gtol=1e-6, ftol=1e-12, history=6, check_every=8, max_eval=None):
        """The minimum of every draw over the box bounds (Dx, 2) = [[low, high], ...], on the device (optimize, DESIGN
        I.17): an optimize.PathOptimum with x (P, Dx), fun (P,), P = N * sample_size, the best of n_starts local optima of
        output `output` of the last layer (maximize: the largest; fun is the draw's own value), and every start's x_all
        (P, R, Dx), fun_all, status, n_iter, n_eval (P, R).  Starts: x0 (R, Dx) shared or (P, R, Dx), projected into the
        box; else per draw the n_starts best of n_candidates rows in the box (np.random.default_rng(seed).uniform, or with
        qmc scipy's scrambled Sobol' sequence, n_candidates a power of two), ties to the lower row.  All P * n_starts
        problems advance in lock-step, a projected L-BFGS with `history` pairs (1 .. 16), until each has a projected
        gradient within gtol, a relative decrease within ftol, maxiter accepted steps or max_eval evaluations (None:
        4 maxiter + 20); the host looks at the count of running problems every check_every rounds.  The same arguments
        give the same bits.  Raises ValueError for an emulator with a likelihood node or a Categorical top and for bad
        bounds, output or n_starts; NotImplementedError for draws made by sample_functions_vecchia (they are only
        piecewise differentiable: use sample_functions)."""
        from . import optimize
        return optimize.minimize(*self._lane_problem(bounds, 'minimize'), bounds, n_starts, n_candidates, output, maximize, x0,
                                 seed, qmc, maxiter, gtol, ftol, history, check_every, max_eval)

    def calibrate(self, y, obs_sd, bounds, n_chains=4, n_samples=500, warmup=500, thin=1, n_candidates=2048, x0=None, seed=None,
                  qmc=False, step=0.1, scale=None, *, controls=None, control_columns=None, obs_cov=None, prior=None, rng='numpy',
                  target_accept=None, method='mala', n_leapfrog=8, jitter=True):
        """The posterior of the input x given an observation of the outputs, for every draw, on the device (calibrate,
        DESIGN I.19): a calibrate.PathPosterior with x (P, R, S, Dx), logp (P, R, S), P = N * sample_size draws, R =
        n_chains chains, S = n_samples samples.  Draw p's chains sample p(x | y, f_p) proportional to prior(x) N(y; f_p(x),
        obs_sd^2) on the box bounds (Dx, 2); result.pooled() weighs all draws equally, which is the MODULAR (cut) posterior
        of Liu, Bayarri and Berger (2009): the emulator's uncertainty enters the calibration, the observation does not
        re-train the emulator.  y: (K,) one value per output of the last layer, or (T, K) replicates at the same unknown x;
        NaN marks an unobserved entry.  obs_sd: a positive scalar or (K,).  prior: None (uniform on the box) or (mean (Dx,),
        sd (Dx,)), independent normals truncated to the box, an infinite sd flat.  The sampler is MALA with the diagonal
        preconditioner scale (Dx,) (default high - low) and a step per chain, `step` at first, adapted over `warmup` rounds
        towards the acceptance rate target_accept and fixed from then on; every thin-th round after warm-up is kept.  A
        proposal outside the box is rejected.  target_accept None: 0.574 for 'mala', 0.8 for 'hmc'.  method='hmc' (DESIGN
        I.20) samples by Hamiltonian Monte Carlo instead: an iteration is a trajectory of n_leapfrog leapfrog steps (with
        jitter, of a length drawn uniformly from 1 .. n_leapfrog per iteration and shared by the chains), one walk
        evaluation each, with the walls of the box reflecting; result.evaluations counts the walk evaluations.
        Starts: x0 (R, Dx) shared or (P, R, Dx), projected into the box; else per draw the n_chains rows of highest posterior density among n_candidates rows in the box (as minimize draws them), ties to
        the lower row.  The normal and uniform draws come from np.random.SeedSequence(seed): the same arguments give the
        same bits, and chain (p, r) does not depend on the chains beside it.  rng='device' makes the normal and uniform numbers on the device instead
        (Philox4x64-10 streams keyed by the seed, DESIGN I.23: other numbers than rng='numpy' gives, as reproducible, and
        particle or chain (p, r)'s own whatever runs beside it); result.rng records it.  result.rhat and result.ess (P, Dx) are the
        split R-hat and the effective sample size per draw; result.summary() the pooled mean and interval.  Raises
        ValueError for an emulator with a likelihood node or a Categorical top and for bad bounds, y, obs_sd or counts;
        NotImplementedError for draws made by sample_functions_vecchia.
        Field data (DESIGN I.24): controls (T, Dc), T <= fieldcal.MAX_SITES, are the known settings of T measurements and
        control_columns their Dc columns of the input; the other columns, in increasing order, are the calibration parameters
        theta, shared by all sites, and everything that described x describes theta: bounds (Dtheta, 2), prior, scale, x0 and
        result.x have Dtheta columns; result.columns names them, result.controls keeps the settings.  y is (T, K), row t
        measured at controls[t] (repeated rows are replicates), NaN unobserved; obs_sd a positive scalar, (K,) or (T, K);
        obs_cov None, (T, T) or (K, T, T): the covariance across the sites of output k's error (a model discrepancy) on top of
        the independent obs_sd^2, the outputs independent of each other.  A covariance that does not factor raises
        ValueError, and so does obs_cov without controls."""
        from . import calibrate, fieldcal
        lane, problem = fieldcal.prepare(self._lane_problem, 'calibrate', y, obs_sd, bounds, controls, control_columns, obs_cov)
        return calibrate.calibrate(*lane, y, obs_sd, bounds, n_chains, n_samples, warmup, thin, n_candidates, x0, seed, qmc, step,
                                   scale, problem=problem, prior=prior, rng=rng, target_accept=target_accept, method=method,
                                   n_leapfrog=n_leapfrog, jitter=jitter)

    def calibrate_smc(self, y, obs_sd, bounds, n_particles=1024, n_moves=4, ess_frac=0.5, max_stages=100, seed=None, step=0.1,
                      scale=None, prior=None, target_accept=0.574, *, controls=None, control_columns=None, obs_cov=None, rng='numpy'):
        """calibrate's posteriors by tempered sequential Monte Carlo, with every draw's evidence, on the device (DESIGN
        I.21): a calibrate.ParticlePosterior with x (P, n_particles, Dx) and log_evidence (P,), the estimate of log of the
        integral of prior(x) exp(ll_p(x)) over the box under the normalised prior.  y, obs_sd, bounds, prior, scale, step
        and target_accept as in calibrate.  Draw p's particles start from the prior on the box; its likelihood is switched
        on in steps of beta in [0, 1], each the largest that keeps the effective sample size of the incremental weights at
        ess_frac of the live particles; a step reweights, resamples systematically and moves every particle by n_moves
        MALA steps under prior(x) exp(beta ll_p(x)), with one step size per draw, `step` at first, set after every stage
        from the stage's acceptance rate towards target_accept.  The particles do not start in a
        mode, so a multimodal posterior keeps its modes in proportion.  At most max_stages steps: a draw still below
        beta = 1 has status max_stages.  n_particles <= calibrate.MAX_PARTICLES.  The random numbers come from
        np.random.SeedSequence(seed); draw p's do not depend on the draws beside it.  rng='device' makes the normal and uniform numbers on the device instead
        (Philox4x64-10 streams keyed by the seed, DESIGN I.23: other numbers than rng='numpy' gives, as reproducible, and
        particle or chain (p, r)'s own whatever runs beside it); result.rng records it.  result.draw_weights() weighs the draws
        by their evidence; result.pooled() stays the modular posterior.  Raises as calibrate does.  controls,
        control_columns and obs_cov: field data as in calibrate; log_norm is then -sum_k (T_k / 2 log 2 pi + sum log diag L_k),
        L_k the factor of output k's covariance over its observed sites, and log_evidence + log_norm still estimates
        log p(y | f_p)."""
        from . import calibrate, fieldcal
        lane, problem = fieldcal.prepare(self._lane_problem, 'calibrate_smc', y, obs_sd, bounds, controls, control_columns, obs_cov)
        return calibrate.calibrate_smc(*lane, y, obs_sd, bounds, n_particles, n_moves, ess_frac, max_stages, seed, step, scale,
                                       prior, target_accept, problem=problem, rng=rng)

    def failure_probability(self, threshold, bounds, output=0, below=False, n_particles=1024, level_prob=0.1, n_moves=4,
                            max_stages=50, min_prob=1e-12, seed=None, step=1.0, prior=None, target_accept=0.44,
                            rng='numpy'):
        """The probability that output `output` of the last layer reaches threshold (below: falls to it) when x is
        distributed over the box bounds (Dx, 2), for every draw, on the device (reliability, DESIGN I.22): a
        reliability.FailureProbability with prob (P,), P = N * sample_size, the estimate of prior{x : f_p(x) >= threshold}
        by subset simulation, every stage's level, conditional probability, acceptance rate and step (P, T), and x
        (P, n_particles, Dx), samples of the prior given the event.  prior: None (uniform on the box) or (mean (Dx,), sd
        (Dx,)), independent normals truncated to the box, as in calibrate.  Draw p's particles start from the prior; a stage
        takes the floor(level_prob n_particles)-th largest value as the next level, clones the particles at or above it
        and moves each n_moves times by component-wise Metropolis steps inside the level set, of width step times the
        survivors' spread per column, the step following the acceptance rate towards target_accept from stage to stage.
        It takes about log(1 / prob) / log(1 / level_prob) stages of n_particles (n_moves + 1) rows each and no gradient.
        At most max_stages stages (status max_stages), and none once the running product is under min_prob (status
        below_min): prob is then an upper bound.  n_particles <= reliability.MAX_PARTICLES.  The random numbers come from
        np.random.SeedSequence(seed); draw p's do not depend on the draws beside it, and the same arguments give the same
        bits.  rng='device' makes the normal and uniform numbers on the device instead
        (Philox4x64-10 streams keyed by the seed, DESIGN I.23: other numbers than rng='numpy' gives, as reproducible, and
        particle or chain (p, r)'s own whatever runs beside it); result.rng records it.  result.summary() gives the predictive probability and its interval over the draws, result.cov() the
        Monte-Carlo error of a draw's own number.  Raises ValueError for an emulator with a likelihood node or a
        Categorical top and for bad bounds, output or counts; NotImplementedError for draws made by
        sample_functions_vecchia."""
        from . import reliability
        return reliability.failure_probability(*self._lane_values(bounds, 'failure_probability'), threshold, bounds, output,
                                               below, n_particles, level_prob, n_moves, max_stages, min_prob, seed, step,
                                               prior, target_accept, rng)

    def _lane_values(self, bounds, what):
        """_lane_problem's sibling for a driver without gradients: (engine, P, K, Dx, values) after the same refusals,
        values the walk at per-path rows (P, R, Dx) -> (P, R, K), no Jacobian."""
        e, P, K, Dx = self._lane_problem(bounds, what)[:4]

        def values(xt):
            for cur, _ in self._walk(xt):
                pass
            return cur.contiguous()
        return e, P, K, Dx, values

    def _lane_problem(self, bounds, what):
        """What minimize and calibrate hand to their drivers after their common refusals: (engine, P, K, Dx, values,
        value_and_jac, width), the closures over the shared-rows walk and the walk at per-path rows."""
        self._check_differentiable()
        _check_smooth(self.nodes.values(), what)
        e, P = self.engine, self.N * self.sample_size
        K, D = max(len(layer) for layer in self.layers), max(nf.Omega.shape[1] for nf in self.nodes.values())
        Dx = np.asarray(bounds).shape[0] if np.ndim(bounds) == 2 else None
        read = max(int(np.max(c)) for l, layer in enumerate(self.layers) for nd in layer
                   for c in ((nd.input_dim if l == 0 else []), ([] if nd.connect is None else nd.connect)) if len(c))
        if Dx is not None and Dx <= read:
            raise ValueError('%s: bounds has %d rows, the emulator reads column %d of its input' % (what, Dx, read))

        def values(xd):
            for cur, _ in self._walk(xd):
                pass
            return cur

        def value_and_jac(xt):
            for cur, J in self._walk(xt, jacobians='last'):
                pass
            return cur, J
        return e, P, len(self.layers[-1]), Dx, values, value_and_jac, 4 * K + 3 * D + 4

    def active_subspace(self, X, bounds=None):
        """The second moment of every draw's input gradient over the rows of X (M, Dx), a host array, M >= 2, Dx <= 64
        (sensitivity.uniform_design makes a uniform sample of a box): a sensitivity.ActiveSubspaceResult with C
        (K, N * sample_size, Dx, Dx), its eigen-decomposition (the active subspace), dgsm and, with bounds (Dx, 2), the
        bound on the total Sobol' indices; K the outputs of the last layer.  The Jacobian of the walk is contracted on the
        device in blocks of rows (DESIGN I.18); the result does not depend on the blocks by a bit.  Columns of X that the
        model does not read give exactly zero rows and columns of C.  Raises ValueError for an emulator with a likelihood
        node or a Categorical top, NotImplementedError for draws made by sample_functions_vecchia."""
        from . import sensitivity
        self._check_differentiable()
        _check_smooth(self.nodes.values(), 'active_subspace', 'it has no gradient to take moments of')
        bounds = sensitivity.check_rows(X, bounds)
        e, P, Dx = self.engine, self.N * self.sample_size, X.shape[1]
        K, D = max(len(layer) for layer in self.layers), max(nf.Omega.shape[1] for nf in self.nodes.values())
        # value_and_grad's doubles per row and path, and the partial sums: NC / 64 per output
        width = 4 * K + 3 * D + 4 + 2 * D + (3 * K + 2) * Dx + -(-len(self.layers[-1]) * sensitivity.n_sums(Dx) // 64)

        def value_and_jac(xd):
            for cur, J in self._walk(xd, jacobians='last'):
                pass
            return cur.contiguous(), J
        sums = sensitivity.gradient_moments(e, value_and_jac, X, P, width)
        if self.after is not None:
            self.after(e, self.nodes.values())
        return sensitivity.ActiveSubspaceResult(sums, len(X), bounds)

    def _block(self, x, noise=False, jacobians=None):
        """The walk at one block of rows: (values, Jacobians), per layer (P, M, K) host arrays and, with jacobians 'last' for
        the last layer or 'all' for every layer, (P, M, K, Dx) ones.  Without jacobians the nodes are evaluated by
        dgpamd_pathfun_eval and no Jacobian is allocated; noise adds every GP node's N(0, scale * nugget) term.
        With them every node's (P, M, D_node) gradient is folded into the Jacobian of its layer with respect to x, on the
        device.  First layer: the gradient scattered into the node's input_dim and connect columns of x.  Deeper:
        J[p, m, :] = sum_k g[p, m, k] J_below[p, m, input_dim[k], :] plus the connect part scattered into x's columns -- one
        fused multiply-add per element and k, in the order of k, so that a row's Jacobian does not depend on the rows that
        share its block (a library contraction may pick another summation order at another size)."""
        vals, jac = [], []
        for l, (cur, J) in enumerate(self._walk(self.engine.tensor(x), noise, jacobians)):
            vals.append(cur.cpu().numpy())
            if jacobians == 'all' or (jacobians == 'last' and l == len(self.layers) - 1):
                jac.append(J.cpu().numpy())
        return vals, jac

    def _walk(self, xd, noise=False, jacobians=None):
        """_block's walk at the rows of the device tensor xd (M, Dx), nothing copied to the host: yields every layer's
        ((P, M, K) values, (P, M, K, Dx) Jacobian or None without jacobians), device tensors.  xd (P, M, Dx): every path
        at M rows of its own (the node kernels' per-path form; optimize.minimize's trial points)."""
        assert not (noise and jacobians), 'the noise term has no derivative'
        e, P = self.engine, self.N * self.sample_size
        assert xd.dim() == 2 or (xd.dim() == 3 and xd.shape[0] == P)
        M, Dx = xd.shape[-2:]
        Js = {}

        def draw(l, k, nodes, xin):
            nd, nf = nodes[0], self.nodes[l, k]
            if jacobians is None:
                out = nf(e, xin)
                if noise:
                    out += nf.noise_sd() * e.tensor(self.rng.standard_normal((P, M)))
                return out
            out, g = nf.value_and_grad(e, xin)
            if l not in Js:
                Js.pop(l - 2, None)
                Js[l] = e.zeros(P, M, len(self.layers[l]), Dx)
            J = Js[l][:, :, k]
            connect = [] if nd.connect is None else list(nd.connect)
            if l == 0:
                _scatter_add(J, g, list(nd.input_dim) + connect)
            else:
                below, kd = Js[l - 1], len(nd.input_dim)
                for i, kk in enumerate(nd.input_dim):
                    J.addcmul_(g[:, :, i, None], below[:, :, int(kk)])
                _scatter_add(J, g[:, :, kd:], connect)
            return out

        for l, cur in enumerate(pathwalk.walk(e, [self.layers] * self.N, self.sample_size, xd, None,
                                              lambda nd: pathwalk.first(xd, nd).contiguous(), draw, own_input=True)):
            yield cur, Js.get(l)


class GpPaths:
    """gp.sample_functions' result: paths(x, noise=False) -> (M, sample_size), column j the j-th posterior draw of the GP as
    a function, evaluated at the rows of x: any number of rows, the same values at the same rows in every call.
    noise=True adds an independent N(0, scale * nugget) term per row and path, np.random.standard_normal((sample_size, M))
    drawn afresh on every call (the nugget that sample_paths' joint covariance carries on its diagonal).
    paths.value_and_grad(x) -> ((M, sample_size), (M, Dx, sample_size)) and paths.grad(x) -> (M, Dx, sample_size), Dx =
    x.shape[1]: entry [m, d, j] = d draw j at row m / d x[m, d], zero in the columns of x that the GP does not read."""

    def __init__(self, model, sample_size, n_features, m=None):
        """m None: the dense draws of sample_functions; else sample_functions_vecchia's, conditioned on the m nearest training
        rows (vpathfun.VecchiaNodePaths: no factor of the training correlation matrix is made)."""
        k = model.kernel
        e = k.engine
        J, F = int(sample_size), int(n_features)
        if J < 1 or F < 1:
            raise ValueError('sample_functions needs sample_size >= 1 and n_features >= 1')
        omega = None if k.rep is None else e.tensor(k.W_diag)
        train = model._joint_train() if m is None else (e.tensor(k._X()), omega)
        n, D = train[0].shape
        draws = list(map(e.tensor, draw_node(np.random, k.name, k.length, D, F, 1, J, n)))
        y = e.tensor(np.asarray(k.output, float).reshape(1, -1))
        self.engine, self.sample_size, self.columns = e, J, model._columns()
        self.input_dim, self.connect = np.array(k.input_dim), None if k.connect is None else np.array(k.connect)
        if m is None:
            self.node = NodePaths.build_shared(e, paths.hyper(k), train, y, omega, draws, J)
        else:
            from . import vpathfun
            self.node = vpathfun.VecchiaNodePaths.build_shared(e, paths.hyper(k), train, y, draws, J, m, 'the gp model')

    def __call__(self, x, noise=False):
        paths.check_2d(x)
        e, J = self.engine, self.sample_size
        xin = x[:, self.columns]
        out = np.concatenate([self.node(e, e.tensor(xb)).cpu().numpy().T
                              for _, xb in _row_blocks(e, xin, J, 2 + xin.shape[1] + self.node.m)], 0)
        if self.node.m:
            from . import vpathfun
            vpathfun.check_status(e, [self.node])
        if noise:
            out = out + self.node.noise_sd() * np.random.standard_normal((J, len(x))).T
        return out

    def value_and_grad(self, x):
        """(values (M, sample_size), gradients (M, Dx, sample_size)) at the rows of x (M, Dx): values bit for bit paths(x)'s,
        gradients[m, d, j] = d draw j at row m / d x[m, d]; the node's gradient is added into its input_dim and connect
        columns of x, every other column is zero."""
        paths.check_2d(x)
        e, J = self.engine, self.sample_size
        xin, (M, Dx) = x[:, self.columns], x.shape
        out, grad = [], np.zeros((M, Dx, J))
        for m0, xb in _row_blocks(e, xin, J, 2 + 3 * xin.shape[1] + Dx):
            f, g = self.node.value_and_grad(e, e.tensor(xb))
            out.append(f.cpu().numpy().T)
            _scatter_add(grad[m0:m0 + len(xb)].transpose(0, 2, 1), g.cpu().numpy().transpose(1, 0, 2), self.columns)
        return np.concatenate(out, 0), grad

    def grad(self, x):
        """value_and_grad(x)[1]."""
        return self.value_and_grad(x)[1]

    def minimize(self, bounds, n_starts=8, n_candidates=2048, output=0, maximize=False, x0=None, seed=None, qmc=False,
                 maxiter=100, gtol=1e-6, ftol=1e-12, history=6, check_every=8, max_eval=None):
        """The minimum of every draw over the box bounds (Dx, 2): PathFunctions.minimize for the sample_size draws of a gp
        model (P = sample_size, one output); a column of x that the GP does not read keeps its start."""
        from . import optimize
        return optimize.minimize(*self._lane_problem(bounds, 'minimize'), bounds, n_starts, n_candidates, output, maximize, x0,
                                 seed, qmc, maxiter, gtol, ftol, history, check_every, max_eval)

    def calibrate(self, y, obs_sd, bounds, n_chains=4, n_samples=500, warmup=500, thin=1, n_candidates=2048, x0=None, seed=None,
                  qmc=False, step=0.1, scale=None, *, controls=None, control_columns=None, obs_cov=None, prior=None, rng='numpy',
                  target_accept=None, method='mala', n_leapfrog=8, jitter=True):
        """The posterior of the input x given an observation y (a number, (1,) or (T, 1) replicates) of the GP's output, for
        every draw: PathFunctions.calibrate for the sample_size draws of a gp model (P = sample_size, one output), the
        modular posterior when pooled; a column of x that the GP does not read is sampled from its prior.  controls,
        control_columns and obs_cov: field data as in PathFunctions.calibrate, y (T,) or (T, 1)."""
        from . import calibrate, fieldcal
        y = np.reshape(y, (-1, 1)) if np.ndim(y) < 2 else y
        lane, problem = fieldcal.prepare(self._lane_problem, 'calibrate', y, obs_sd, bounds, controls, control_columns, obs_cov)
        return calibrate.calibrate(*lane, y, obs_sd, bounds, n_chains, n_samples, warmup, thin, n_candidates, x0, seed, qmc, step,
                                   scale, problem=problem, prior=prior, rng=rng, target_accept=target_accept, method=method,
                                   n_leapfrog=n_leapfrog, jitter=jitter)

    def calibrate_smc(self, y, obs_sd, bounds, n_particles=1024, n_moves=4, ess_frac=0.5, max_stages=100, seed=None, step=0.1,
                      scale=None, prior=None, target_accept=0.574, *, controls=None, control_columns=None, obs_cov=None, rng='numpy'):
        """PathFunctions.calibrate_smc for the sample_size draws of a gp model (P = sample_size, one output; y as in
        calibrate): tempered SMC particles of every draw's posterior and its evidence."""
        from . import calibrate, fieldcal
        y = np.reshape(y, (-1, 1)) if np.ndim(y) < 2 else y
        lane, problem = fieldcal.prepare(self._lane_problem, 'calibrate_smc', y, obs_sd, bounds, controls, control_columns, obs_cov)
        return calibrate.calibrate_smc(*lane, y, obs_sd, bounds, n_particles, n_moves, ess_frac, max_stages, seed, step, scale,
                                       prior, target_accept, problem=problem, rng=rng)

    def failure_probability(self, threshold, bounds, output=0, below=False, n_particles=1024, level_prob=0.1, n_moves=4,
                            max_stages=50, min_prob=1e-12, seed=None, step=1.0, prior=None, target_accept=0.44,
                            rng='numpy'):
        """PathFunctions.failure_probability for the sample_size draws of a gp model (P = sample_size, one output): every
        draw's probability of reaching threshold over the box, by subset simulation; a column of x that the GP does not read
        moves under its prior alone."""
        from . import reliability
        return reliability.failure_probability(*self._lane_values(bounds, 'failure_probability'), threshold, bounds, output,
                                               below, n_particles, level_prob, n_moves, max_stages, min_prob, seed, step,
                                               prior, target_accept, rng)

    def _lane_values(self, bounds, what):
        """PathFunctions._lane_values for the one node of a gp model."""
        e, J, K, Dx = self._lane_problem(bounds, what)[:4]
        cols = torch.as_tensor(self.columns, device=e.device)

        def values(xt):
            return self.node(e, xt[:, :, cols].contiguous())[:, :, None].contiguous()
        return e, J, K, Dx, values

    def _lane_problem(self, bounds, what):
        """PathFunctions._lane_problem for the one node of a gp model."""
        _check_smooth([self.node], what)
        e, J = self.engine, self.sample_size
        cols = torch.as_tensor(self.columns, device=e.device)

        def values(xd):
            return self.node(e, xd[:, cols].contiguous())[:, :, None]

        def value_and_jac(xt):
            f, g = self.node.value_and_grad(e, xt[:, :, cols].contiguous())
            jac = e.zeros(*xt.shape)
            _scatter_add(jac, g, self.columns)
            return f[:, :, None], jac[:, :, None]
        Dx = np.asarray(bounds).shape[0] if np.ndim(bounds) == 2 else None
        if Dx is not None and Dx <= int(np.max(self.columns)):
            raise ValueError('%s: bounds has %d rows, the model reads column %d' % (what, Dx, int(np.max(self.columns))))
        return e, J, 1, Dx, values, value_and_jac, 2 + len(self.columns)

    def active_subspace(self, X, bounds=None):
        """PathFunctions.active_subspace for the sample_size draws of a gp model: a sensitivity.ActiveSubspaceResult without
        the output axis, C (sample_size, Dx, Dx), dgsm (Dx, sample_size), ...; a column of X that the GP does not read gives
        exactly zero rows and columns of C."""
        from . import sensitivity
        _check_smooth([self.node], 'active_subspace', 'it has no gradient to take moments of')
        bounds = sensitivity.check_rows(X, bounds)
        e, J, Dx = self.engine, self.sample_size, X.shape[1]
        if Dx <= int(np.max(self.columns)):
            raise ValueError('active_subspace: X has %d columns, the model reads column %d' % (Dx, int(np.max(self.columns))))

        def value_and_jac(xd):
            f, g = self.node.value_and_grad(e, pathwalk.cols(xd, self.columns).contiguous())
            jac = e.zeros(J, xd.shape[0], Dx)
            _scatter_add(jac, g, self.columns)
            return f[:, :, None], jac[:, :, None]
        # value_and_grad's doubles per row and path, the Jacobian in x's columns, and the partial sums
        width = 2 + 3 * len(self.columns) + 2 * Dx + -(-sensitivity.n_sums(Dx) // 64)
        return sensitivity.ActiveSubspaceResult(sensitivity.gradient_moments(e, value_and_jac, X, J, width), len(X), bounds,
                                                squeeze=True)

    def sobol(self, A, B):
        """Sobol' indices of every draw from the base samples A, B (n_base, Dx), host arrays of one shape, n_base >= 2: a
        sensitivity.SobolResult with first and total (Dx, sample_size); a column of x that the GP does not read gets exactly 0.
        Evaluated in blocks of rows and summed on the device; the result does not depend on the blocks by a bit."""
        from . import sensitivity
        sensitivity.check_design(A, B)
        e, J = self.engine, self.sample_size

        def evaluate(xd):
            return self.node(e, pathwalk.cols(xd, self.columns).contiguous())[:, :, None]
        sums = sensitivity.pick_freeze(e, evaluate, A, B, J, 2 + len(self.columns) + self.node.m + 3 + 3 * A.shape[1])
        if self.node.m:
            from . import vpathfun
            vpathfun.check_status(e, [self.node])
        return sensitivity.SobolResult(sums, len(A), squeeze=True)
