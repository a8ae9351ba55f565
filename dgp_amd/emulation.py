"""Prediction from a trained DGP by stochastic imputation -- mirror of dgpsi.emulator
(emulation.py:24-44 construction, :631-854 predict(method='mean_var')).

Construction draws the N imputations from one ESS chain after a burn-in
(emulation.py:31-44).  Instead of deep-copying the whole structure with an n x n
R^-1 (and D n x n Psexp) per node per imputation, the emulator keeps per
imputation only the latent columns and builds device-resident statistics:
  * first-layer nodes: inputs and hyper-parameters are identical in every
    imputation, so R^-1 is factored ONCE and the N vectors R^-1 y_s ride along as
    right-hand sides of that single factorisation; the predictive variance is
    shared, only the mean differs;
  * deeper nodes: one factorisation per imputation (their inputs differ).
`predict` walks the layers on the device and accumulates the imputation moments
mu = mean_s mu_s, var = mean_s(mu_s^2 + v_s) - mu^2 (emulation.py:846-847) in place.

Multi-GPU: with torch.distributed initialised, each rank draws its share of the N
imputations from its own chain (own burn-in) and one all-reduce(sum) of the two
moment arrays precedes the finalisation (RCCL over xGMI on the GPU box).
"""
import contextlib
import copy

import collections
import os

import numpy as np
from .kernel_class import bind_private, peek
import torch

from .imputation import imputer, DrawStream
from .ops import default_engine
from . import dist as ddist, paths, pathwalk


class _LazyPer:
    """The per-imputation prediction statistics of a linked GP node (R^-1, R^-1 y, its inputs: kernel_class.py:735-764 for
    every imputation, emulation.py:43), built when first asked for and kept while the emulator's byte budget allows.
    The reference holds all of them; at BASELINE configs[2]'s size -- 50 imputations x 3 nodes, n = 5000 -- that is 31 GB of
    inverses of which a predict() call uses each exactly once, and rebuilding one costs ~30 ms against the seconds its pair
    kernel runs.  Budget: DGPAMD_STATS_GB (default 16); smaller models never evict."""

    def __init__(self, owner, key, build, nbytes):
        self.owner, self.key, self.build, self.nbytes = owner, key, build, int(nbytes)

    def __getitem__(self, s):
        o = self.owner
        ck = self.key + (int(s),)
        hit = o._per_cache.get(ck)
        if hit is not None:
            o._per_cache.move_to_end(ck)
            return hit
        budget = float(os.environ.get('DGPAMD_STATS_GB', '16')) * 2 ** 30
        while o._per_cache and o._per_bytes + self.nbytes > budget:
            _, old = o._per_cache.popitem(last=False)
            o._per_bytes -= old['_bytes']
        item = self.build(int(s))
        item['_bytes'] = self.nbytes
        o._per_cache[ck] = item
        o._per_bytes += self.nbytes
        return item


def _host(per_layer):
    """_layer_moments' device pairs as numpy arrays."""
    return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in per_layer]


def _mice_var(e, x, x_extra, nd, nugget_s):
    """functions.mice_var (functions.py:244-256) on the device: scale / diag(R^-1) of the correlation matrix of
    the candidate set (smoothing nugget max(nugget_s, nugget)).  pinvh in the reference; a Cholesky-based
    inverse here (R is positive definite for any positive nugget)."""
    Xin = x[:, nd.input_dim]
    if nd.connect is not None:
        Xin = np.concatenate((Xin, x_extra[:, nd.connect]), 1)
    n = len(Xin)
    Np = e.padded_dim(n)
    A, Ainv = e.empty(Np, Np), e.empty(Np, Np)
    e.kmatrix(nd.name, e.tensor(Xin), None, None, nd.length, max(nugget_s, nd.nugget[0]), out=A, full=False)
    work = e.potrf_workspace(n, 1)
    _, info = e.potrf(n, A, work=work)
    e.potri(n, A, Ainv, 0, work)
    if int(e.fetch(info)[0]):
        raise np.linalg.LinAlgError('candidate-set correlation matrix is not positive definite')
    d = torch.diagonal(Ainv)[:n]
    return (float(nd.scale[0]) / d).cpu().numpy()


class emulator:
    """Args as dgpsi.emulator (emulation.py:24): all_layer (from dgp.estimate()), N, block;
    plus `seed`, `device` and `shard`: None / True / False -- the N imputations are split over the ranks of an
    initialised torch.distributed group (None: iff there is one) and predictions cost one all-reduce of the two moment
    sums; 'points' -- every rank holds all N imputations (same seed, same chain) and predict() splits the rows of x over
    the ranks instead, one all-gather of the results (what ppredict's pool did, emulation.py:578-629)."""

    def __init__(self, all_layer, N=10, block=True, seed=None, device=None, shard=None):
        self.all_layer = all_layer
        self.n_layer = len(all_layer)
        self.vecch = bool(all_layer[0][0].vecch)
        self.N_total = int(N)
        self.shard_points = shard == 'points' and ddist.is_active()
        self.shard = False if shard == 'points' else (ddist.is_active() if shard is None else bool(shard))
        rank, world = (ddist.rank(), ddist.world()) if self.shard else (0, 1)
        if self.shard and self.N_total < world:   # (a rank without imputations would skip the collectives the others enter)
            raise Exception('emulator(shard=True) needs at least one imputation per rank: N = %d < %d ranks' % (self.N_total, world))
        self.engine = default_engine(device)
        for layer in all_layer:
            for nd in layer:
                if nd.type == 'gp':
                    nd.engine = self.engine
        self.N = ddist.share(self.N_total, rank, world)
        if self.shard_points and seed is None:      # all ranks must draw the same imputations: rank 0's entropy for everyone
            seed = ddist.broadcast_int(np.random.SeedSequence().entropy, src=0, device=self.engine.device)   # (no pickling: RCCL moves device words)
        ss = np.random.SeedSequence(seed)
        self.imp = imputer(all_layer, block, draws=DrawStream(ss.spawn(world)[rank]), engine=self.engine)
        self._sample_rng = np.random.default_rng(ss.spawn(world)[rank])   # predict(method='sampling')
        if self.vecch:
            self.imp.update_ord_nn()
            self.imp.sample(burnin=20)
        else:
            self.imp.sample(burnin=50)
        # per imputation: the latent columns of every hidden layer (n x M_l), small
        self.latents = []
        self.orders = []
        for _ in range(self.N):
            if self.vecch:
                self.imp.update_ord_nn()
            self.imp.sample()
            self.latents.append([np.stack([np.asarray(nd.output, float).reshape(-1) for nd in layer], 1)
                                 for layer in all_layer[:-1]])
            if self.vecch:
                self.orders.append([[(nd.ord.copy(), nd.NNarray.copy()) if nd.type == 'gp' else None for nd in layer]
                                    for layer in all_layer])
        self._stats = None

    def to_vecchia(self):
        """Switch the emulator to Vecchia predictions (emulation.py:63-74): every node conditions on its nearest training
        points instead of using stored n x n statistics."""
        if self.vecch:
            raise Exception('The DGP emulator is already in Vecchia mode.')
        self.vecch = True
        for layer in self.all_layer:
            for nd in layer:
                if nd.type == 'gp':
                    nd.vecch = True
        self._stats = None

    def remove_vecchia(self):
        """Back to dense predictions (emulation.py:76-88); the statistics are rebuilt on the next predict()."""
        if not self.vecch:
            raise Exception('The DGP emulator is already in non-Vecchia mode.')
        self.vecch = False
        for layer in self.all_layer:
            for nd in layer:
                if nd.type == 'gp':
                    nd.vecch = False
        self._stats = None

    def __getstate__(self):
        st = dict(self.__dict__)
        st['engine'] = None       # device context and statistics are rebuilt after unpickling (utils.write / read)
        st['_stats'] = None
        st.pop('_per_cache', None)
        st.pop('_per_bytes', None)
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self.engine = default_engine()
        for layer in self.all_layer:
            for nd in layer:
                if nd.type == 'gp':
                    nd.engine = self.engine
        self.imp._engine = self.engine

    # dgpsi keeps `all_layer_set`: N deep copies of the structure.  Built on demand (arrays only, no R^-1).
    @property
    def all_layer_set(self):
        out = []
        for s in range(self.N):
            out.append(self._structure(s))
        return out

    def _structure(self, s):
        al = copy.deepcopy(self.all_layer)
        lat = self.latents[s]
        for l, layer in enumerate(al):
            for k, nd in enumerate(layer):
                if l < self.n_layer - 1:
                    nd.output = lat[l][:, [k]].copy()
                if l > 0:
                    bind_private(nd, 'input', lat[l - 1][:, nd.input_dim].copy())
        return al

    # ------------------------------------------------------------------ statistics
    def _build_stats(self):
        """R^-1 (device, ld = Np) and R^-1 y for every GP node and imputation."""
        e = self.engine
        S = self.N
        stats = {}
        for l, layer in enumerate(self.all_layer):
            for k, nd in enumerate(layer):
                if nd.type != 'gp':
                    continue
                n = len(nd.output)
                Np = e.padded_dim(n)
                cap = Np - n
                Xg = None if peek(nd, 'global_input') is None else e.tensor(peek(nd, 'global_input'))
                W = None if nd.rep is None else e.tensor(nd.W_diag)

                def factor(Xl, Y, nd=nd, Xg=Xg, W=W):
                    return paths.inverse_with_rhs(e, nd.name, Xl, Xg, W, nd.length, nd.nugget[0], Y, 'emuA')

                if l == 0:
                    Xl = e.tensor(peek(nd, 'input'))
                    rys, Rinv = [], None
                    for c0 in range(0, S, cap):   # all imputations' y as right-hand sides of ONE factorisation
                        Y = e.tensor(np.stack([self._ys(s, l, k) for s in range(c0, min(S, c0 + cap))]))
                        Rinv, ry = factor(Xl, Y)
                        rys.append(ry)
                    stats[(l, k)] = dict(shared=True, Rinv=Rinv, ld=Np, ry=torch.cat(rys), n=n, Wall=e.tensor(nd._X()))
                else:
                    def build(s, l=l, k=k, nd=nd, factor=factor, Xg=Xg):   # (defaults: called after this loop has moved on)
                        Xin = self._train_in(s, l, nd)
                        Rinv, ry = factor(e.tensor(Xin), e.tensor(self._ys(s, l, k)[None, :]))
                        cells = e.linkgp_cells(nd.name, Xin, Xg, Rinv, ry[0])   # (Matern: training points grouped by cells)
                        return cells if cells is not None else dict(Rinv=Rinv, ry=ry[0].contiguous(), W=e.tensor(Xin))
                    stats[(l, k)] = dict(shared=False, per=_LazyPer(self, (l, k), build, Np * Np * 8), ld=Np, n=n, Wg=Xg)
        self._stats = stats
        self._per_cache = collections.OrderedDict()
        self._per_bytes = 0

    def _layer_moments(self, x, mode='dense', m=None):
        """Per layer the (mean, variance) of every node at the rows of x for every imputation held by this rank, as
        device tensors (S, M, K) -- the layer walk of emulation.py:701-779 (pathwalk.moments); the mode is what a GP node
        does with its inputs: 'dense' the stored statistics; 'loo' the same with test row k leaving out training row k;
        'vecchia' no stored statistics, the node's m nearest training points (kernel_class.py:603-619,647-664)."""
        e = self.engine
        if mode != 'vecchia' and self._stats is None:
            self._build_stats()
        xd = e.tensor(x)
        node = self._node_vecchia(m) if mode == 'vecchia' else lambda *a: self._node_dense(*a, loo=mode == 'loo')
        return list(pathwalk.moments(e, [self.all_layer] * self.N, xd, None, None,
                                     lambda nd: pathwalk.Inputs(pathwalk.first(xd, nd).contiguous(), None, None), node))

    def _node_dense(self, l, k, nodes, inp, loo=False):
        """pathwalk.moments' node predictor on the stored statistics.  loo: every node conditions on all training points
        but its own (emulation.py:90-143 with vecch False: test row k leaves out training row k at every layer, which is
        what get_pred_nn's all-points shortcut (vecchia.py:23-26) followed by kernel_class.py:610-611,655-656 does).  Nothing
        is refactorised: first-layer nodes use the block-inverse identities  mean = y_d - (R^-1 y)_d / (R^-1)_dd,
        var = scale (1 / (R^-1)_dd + nugget (1 - W_d));  linked nodes go through dgpamd_linkgp_loo, which applies the
        rank-one downdate of R^-1 inside the pair weights."""
        e, nd, st, S = self.engine, nodes[0], self._stats[(l, k)], self.N
        n = st['n']
        if l == 0 and loo:
            if inp.m.shape[0] != n or not torch.equal(st['Wall'], inp.m):
                raise Exception('loo: the rows of X must be the training input positions of the emulator, in order.')
            rho = st['Rinv'][:n, :n].diagonal()
            wd = 1.0 if nd.rep is None else e.tensor(nd.W_diag)
            Y = e.tensor(np.stack([self._ys(s, l, k) for s in range(S)]))
            return Y - st['ry'] / rho, nd.scale[0] * (1.0 / rho + nd.nugget[0] * (1.0 - wd))
        if l == 0:
            return e.gp_predict(nd.name, inp.m, st['Wall'], nd.length, st['Rinv'], st['ld'], st['ry'], nd.scale[0], nd.nugget[0])
        mean, var = e.empty(S, inp.m.shape[1]), e.empty(S, inp.m.shape[1])
        for s in range(S):
            ps = st['per'][s]
            drop = None if not loo else ps['pos'] if 'pos' in ps else torch.arange(n, device=e.device, dtype=torch.int32)
            e.linkgp_predict(nd.name, inp.m[s], inp.v[s], inp.z, ps['W'], ps.get('Wg', st['Wg']), nd.length, ps['Rinv'], st['ld'],
                             ps['ry'], nd.scale[0], nd.nugget[0], mean=mean[s], var=var[s], drop=drop)
        return mean, var

    def _node_vecchia(self, m):
        """pathwalk.moments' node predictor in Vecchia mode: every node conditions on its m nearest training points, the
        imputation's own latents below the first layer.
        Conditioning sets are searched once per GROUP of nodes that must get the same ones: nodes of a layer with the same
        input columns and ONE shared lengthscale see the same points in the same (distance, index) order whatever the
        lengthscale's value (a uniform scaling; the reference itself shares orderings between such siblings in training,
        imputation.py:245-262) -- and in the first layer also across imputations, whose inputs are the same X.  At
        BASELINE configs[3] (8 + 1 nodes, 2 imputations) that is 3 searches instead of 18, which were 60 % of a large
        Vecchia prediction.  DGPAMD_NN_SHARE=0 searches per node like the reference (vecchia.py:20-40 per gp_prediction)."""
        e, S = self.engine, self.N
        share = os.environ.get('DGPAMD_NN_SHARE', '1') != '0'
        nn_sets = {}

        def node(l, k, nodes, inp):
            nd = nodes[0]
            nd.pred_m = m
            mean, var = e.empty(S, inp.m.shape[-2]), e.empty(S, inp.m.shape[-2])
            for s in range(S):
                train = (nd._X() if l == 0 else self._train_in(s, l, nd, True), self._ys(s, l, k))
                ms = inp.m if l == 0 else inp.m[s]
                nn = None
                if share and not nd.loo_state:
                    key = (l, None if l == 0 else s, tuple(np.asarray(nd.input_dim).tolist()),
                           None if nd.connect is None else tuple(np.asarray(nd.connect).tolist()),
                           'iso' if len(nd.length) == 1 else tuple(nd.length.tolist()))
                    if key not in nn_sets:
                        nn_sets[key] = nd._pred_nn(ms if inp.z is None else torch.cat((ms, inp.z), 1), train[0])
                    nn = nn_sets[key]
                mean[s], var[s] = nd.predict_at(ms, nn, train) if l == 0 else nd.predict_link(ms, inp.v[s], inp.z, nn, train)
            return mean, var
        return node

    def _cat(self):
        """The Categorical likelihood node of the final layer, or None.  For it the last layer's moments are those of
        its feeding latents (emulation.py:711-716,751-752): they are aggregated over the imputations first and turned
        into class probabilities afterwards."""
        nd = self.all_layer[-1][0]
        return nd if getattr(nd, 'name', None) == 'Categorical' else None

    # ------------------------------------------------------------------ prediction
    def predict(self, x, method='mean_var', full_layer=False, sample_size=50, m=50, aggregation=True):
        """Mean and variance at the rows of x (emulation.py:631-854, method='mean_var').
        Returns (mu, sigma2) as numpy arrays (M x D_out), or per-layer lists if full_layer, or the
        per-imputation lists if aggregation=False."""
        if x.ndim == 1:
            raise Exception('The testing input has to be a numpy 2d-array')
        if method not in ('mean_var', 'sampling'):
            raise Exception("method must be either 'mean_var' or 'sampling'.")
        if getattr(self, 'shard_points', False) and not getattr(self, '_in_points', False):
            return self._predict_points(x, method, full_layer, sample_size, m, aggregation)
        if not self.vecch and self.shard and (method == 'sampling' or not aggregation):
            # (each rank holds its own imputations only: the per-imputation lists / draws would silently be partial)
            raise NotImplementedError("with the imputations sharded over ranks predict() returns aggregated moments only; "
                                      "use emulator(..., shard=False) or shard='points' for method='sampling' / aggregation=False")
        per_layer = self._layer_moments(x, self._mode(), m)
        if method == 'sampling':
            return self._draw_samples(_host(per_layer), sample_size, full_layer)
        return self._aggregate(per_layer, full_layer, aggregation)

    def _mode(self):
        return 'vecchia' if self.vecch else 'dense'

    def _dist_refusals(self, what):
        """What predict_dist and loo_dist refuse: a final layer whose predictive distribution is no mixture of Gaussians, and
        imputations spread over ranks (each rank would build the mixture of its own share)."""
        if self._cat() is not None or any(nd.type == 'likelihood' for nd in self.all_layer[-1]):
            raise ValueError('%s: with a likelihood node in the final layer the predictive distribution is not a mixture of '
                             "Gaussians; draw from it with predict(method='sampling')" % what)
        if self.shard or getattr(self, 'shard_points', False):
            raise NotImplementedError("with the imputations sharded over ranks %s() would return a partial mixture; "
                                      "use emulator(..., shard=False)" % what)

    def predict_dist(self, x, m=50):
        """The predictive distribution itself at the rows of x: the equal-weight mixture of the N imputations' Gaussians as a
        mixture.PredictiveMixture -- mean() and var() are predict(x)'s, bit for bit; cdf, sf, logpdf, quantile, interval and crps
        are evaluated exactly on the device (DESIGN I.15).  Dense and Vecchia-mode emulators (m: the conditioning-set size);
        GP hierarchies only: a likelihood node or a Categorical top raises ValueError."""
        from . import mixture
        mixture.check_points(x)
        self._dist_refusals('predict_dist')
        return mixture.PredictiveMixture(self.engine, *self._layer_moments(x, self._mode(), m)[-1])

    def loo_dist(self, X, m=30):
        """loo(X)'s leave-one-out predictive distributions as a mixture.PredictiveMixture (one row per row of X, replicated rows
        as loo returns them): PIT values are cdf(Y), interval coverage and the leave-one-out CRPS one call each."""
        from . import mixture
        self._dist_refusals('loo_dist')
        return mixture.PredictiveMixture(self.engine, *self._loo_moments(X, m)[-1])

    def _host_moments(self, x, m):
        """_layer_moments in the emulator's own mode as numpy arrays (metric, nllik)."""
        return _host(self._layer_moments(x, self._mode(), m))

    def _aggregate(self, per_layer, full_layer=False, aggregation=True):
        """predict's result from the layers' moments: mu = mean_s mu_s, var = mean_s(mu_s^2 + v_s) - mu^2 over the
        imputations (emulation.py:846-847; summed on the device, over all ranks under `shard`), of the last layer or with
        full_layer of every layer; without either the last layer's per-imputation lists.  A Categorical top turns its
        feeding latents' moments into class probabilities last."""
        e, cat, S = self.engine, self._cat(), self.N
        if not aggregation and not full_layer:
            mu_s, v_s = (list(t.cpu().numpy()) for t in per_layer[-1])
            if cat is not None:
                pr = [cat.prediction(a, b) for a, b in zip(mu_s, v_s)]
                return [p[0] for p in pr], [p[1] for p in pr]
            return mu_s, v_s
        outs = []
        for mean, var in (per_layer if full_layer else per_layer[-1:]):
            s1, s2 = e.zeros(*mean.shape[1:]), e.zeros(*mean.shape[1:])
            for s in range(S):
                e.moments_accumulate(mean[s].contiguous(), var[s].contiguous(), s1, s2)
            if self.shard:
                ddist.allreduce_sum(s1, s2)
            e.moments_finalize(self.N_total if self.shard else S, s1, s2)
            outs.append((s1.cpu().numpy(), s2.cpu().numpy()))
        if cat is not None:
            outs[-1] = cat.prediction(outs[-1][0], outs[-1][1])
        if full_layer:
            return [o[0] for o in outs], [o[1] for o in outs]
        return outs[0]

    def _draw_samples(self, per_layer, sample_size, full_layer):
        """method='sampling' (emulation.py:780-822, GP hierarchies): per imputation and layer the outputs are drawn
        from N(mu_s, sigma2_s), sample_size times.  per_layer: [(mean (S,M,K), var (S,M,K))] as numpy arrays.
        Returns, like the reference, a list over the final layer's nodes of (M x S*sample_size) arrays, or with
        full_layer a list over layers of such lists."""
        rng = self._sample_rng
        lik = any(nd.type == 'likelihood' for nd in self.all_layer[-1])
        out, prev = [], None
        for li, (mean, var) in enumerate(per_layer):
            last = li == len(per_layer) - 1
            if not (full_layer or last or (lik and li == len(per_layer) - 2)):
                continue
            S, M, K = mean.shape
            mu_r, sd_r = np.repeat(mean, sample_size, axis=0), np.repeat(np.sqrt(var), sample_size, axis=0)
            draws = rng.normal(mu_r, sd_r)                       # (S*ss, M, K)
            if last and self._cat() is not None:   # class probabilities at draws of the feeding latents (all columns at once)
                cat = self._cat()
                draws = np.stack([cat.sampling(prev[j][:, cat.input_dim]) for j in range(prev.shape[0])])
            elif last and lik:   # likelihood nodes sample y from draws of their feeding latents (emulation.py:785-822)
                for k, nd in enumerate(self.all_layer[-1]):
                    if nd.type == 'likelihood':
                        for j in range(draws.shape[0]):
                            draws[j, :, k] = nd.sampling(prev[j][:, nd.input_dim])
            prev = draws
            if full_layer or last:
                out.append(list(draws.transpose(2, 1, 0)))
        return out if full_layer else out[0]

    def sample_paths(self, x, sample_size=50, full_layer=False):
        """Joint posterior draws of the emulated function at the rows of x (dense emulators).  Returns the container of
        predict(x, method='sampling'): a list over the final layer's nodes of (M, N*sample_size) arrays, or with full_layer
        a list over layers of such lists -- but column s*sample_size + j is ONE draw over all M rows: path j of
        imputation s.  Each path walks the layers: a first-layer GP node is drawn jointly from its posterior at x; a
        deeper one is conditioned on imputation s's latents and drawn jointly at that path's outputs of the layer below
        (its input_dim columns, plus x[:, connect]); likelihood nodes sample from the path's latents (nd.sampling, or
        cat.sampling for a Categorical node).  Normals come from the emulator's sampling generator, layer by layer and
        node by node, one standard_normal((N, sample_size, M)) block per GP node.  At most 8192 rows of x; an imputation
        whose training correlation matrix is not positive definite raises numpy.linalg.LinAlgError."""
        self._need_dense_unsharded()
        paths.check_points(x)
        e, rng, drawer = self.engine, self._sample_rng, paths.Dense()
        M, S, J = len(x), self.N, int(sample_size)

        def draw(l, k, nd, xin):
            Z = e.tensor(rng.standard_normal((S, J, M)).reshape(S * J, M))
            st = self._joint_stats(l, k)
            if l == 0:
                return drawer.draw_shared(e, paths.hyper(nd), xin, (st['W'], st['Linv']), st['Y'], Z, J)
            out = e.empty(S * J, M)
            for s in range(S):   # (one call per imputation: its L^-1 is passed as it lies; a grouped call stacks copies)
                ps, mine = st['per'][s], slice(s * J, (s + 1) * J)
                out[mine] = drawer.draw_per_path(e, paths.hyper(nd), xin[mine], (ps['W'], ps['Linv']), ps['y'], Z[mine])
            return out
        return self._walk_paths(x, J, full_layer, draw)

    def _need_dense_unsharded(self):
        """What sample_paths and sample_functions refuse: both work on the dense statistics of all N imputations."""
        if self.vecch:
            raise NotImplementedError('sample_paths needs a dense emulator: joint draws of a Vecchia emulator need a sparse '
                                      'algorithm of their own (use remove_vecchia())')
        if self.shard or getattr(self, 'shard_points', False):
            raise NotImplementedError("sample_paths with the imputations sharded over ranks would return partial draws; use "
                                      "emulator(..., shard=False)")

    def sample_functions(self, sample_size=50, n_features=2048):
        """N * sample_size posterior draws of the emulated function as functions (pathwise conditioning, DESIGN I.12):
        returns a pathfun.PathFunctions, paths(x, full_layer=False, noise=False), that evaluates every draw at the rows of
        any x, any number of times, in sample_paths' container and column layout (column s * sample_size + j is path j of
        imputation s).  Each GP node's prior is drawn through n_features random Fourier features shared by the node's paths
        and conditioned on the training set -- the imputation's latents below layer 1 -- by Matheron's rule; the mean of
        the draws is the posterior mean for every n_features, their covariance tends to sample_paths' as n_features
        grows.  Creating the paths costs two triangular products per path; evaluating them (n + n_features) * M * D per
        node and path, rows independent.  What is random in a path is drawn here, from the emulator's sampling generator,
        per GP node in walk order (layer by layer, node by node): standard_normal((n_features, D)) for the frequencies;
        for 'matern2.5' chisquare(5, (n_features, D)); uniform(0, 2 pi, n_features) for the phases;
        standard_normal((N, sample_size, n_features)) for the feature weights; standard_normal((N, sample_size, n)) for the
        nugget term.  Only the samples of likelihood nodes and of a Categorical top (the nodes' own sampling(), on numpy's
        global generator) and the noise=True term (this generator) are drawn afresh on each evaluation (see PathFunctions).  Dense, unsharded emulators, as sample_paths; an imputation whose
        training correlation matrix is not positive definite raises numpy.linalg.LinAlgError naming its layer, node and
        imputation."""
        from . import pathfun
        self._need_dense_unsharded()
        return pathfun.PathFunctions(self, sample_size, n_features)

    def sample_functions_vecchia(self, sample_size=50, n_features=2048, m=50):
        """sample_functions by local conditioning (vpathfun, DESIGN I.14), for dense and Vecchia emulators and any number of
        training rows: the same object, call signatures, container, column layout, noise=True term and handling of
        likelihood nodes and a Categorical top, from the same draws in the same order (equal generator states give the
        features, feature weights and nugget normals of sample_functions).  Each GP node's prior draw is conditioned, row by
        row, on the m nearest training rows of the row (coordinates divided by the lengths; the imputation's latents
        below layer 1) -- the predictor of a Vecchia emulator with Matheron's rule carried through it -- so creation keeps
        nothing n x n and factors nothing, and a row costs O(m^3) whatever n is.  The mean of the draws is the Vecchia
        predictive mean with conditioning sets of m for every n_features, their variance tends to its variance; with m >= n
        the draws are sample_functions'.  A draw is a deterministic function of x (the same values at the same rows in any
        call or split of the rows) but only piecewise smooth: it jumps where a row's nearest training rows change, by about
        the Vecchia error, and paths.grad / paths.value_and_grad raise NotImplementedError.  A conditioning block that does
        not factor is rebuilt with a jitter, row by row (one RuntimeWarning per evaluation call), then raises
        numpy.linalg.LinAlgError naming its layer, node and imputation."""
        from . import pathfun, vpathfun, vpaths
        if self.shard or getattr(self, 'shard_points', False):
            raise NotImplementedError("sample_paths_vecchia with the imputations sharded over ranks would return partial "
                                      "draws; use emulator(..., shard=False)")
        vpaths.check_m(m)
        return pathfun.PathFunctions(self, sample_size, n_features, vpathfun.emulator_nodes(self, sample_size, n_features, m),
                                     vpathfun.check_status)

    def sobol(self, bounds, n_base=4096, sample_size=20, n_features=2048, seed=None, qmc=False, m=50):
        """Sobol' sensitivity indices of the emulated function over the box bounds (Dx, 2), with their posterior
        uncertainty (sensitivity, DESIGN I.16): draws N * sample_size functions -- sample_functions for a dense emulator,
        sample_functions_vecchia(m=m) for one in Vecchia mode, with their refusals -- makes the base samples
        sensitivity.saltelli_design(bounds, n_base, seed, qmc) and returns paths.sobol(A, B), a sensitivity.SobolResult:
        first and total (K, Dx, N * sample_size), one first-order and one total-order index per output, input and draw;
        result.summary() gives their means and intervals over the draws.  Emulators of GP nodes only (ValueError)."""
        from . import pathfun, sensitivity
        pathfun.check_pick_freeze(self.all_layer)
        A, B = sensitivity.saltelli_design(bounds, n_base, seed, qmc)
        if self.vecch:
            fun = self.sample_functions_vecchia(sample_size, n_features, m)
        else:
            fun = self.sample_functions(sample_size, n_features)
        return fun.sobol(A, B)

    def active_subspace(self, bounds, n_rows=4096, sample_size=20, n_features=2048, seed=None, qmc=False):
        """The active subspace and the derivative-based sensitivity measures of the emulated function over the box bounds
        (Dx, 2), with their posterior uncertainty (sensitivity, DESIGN I.18): draws N * sample_size functions
        (sample_functions, with its refusals), makes the design sensitivity.uniform_design(bounds, n_rows, seed, qmc) and
        returns paths.active_subspace(X, bounds), a sensitivity.ActiveSubspaceResult: per output and draw C = E_x[grad f
        grad f^T] (K, N * sample_size, Dx, Dx), the eigenvalues and eigenvectors of the box-normalised C, dgsm and
        total_bound >= the total Sobol' index (K, Dx, N * sample_size); result.subspace(k) gives the mean subspace and every
        draw's distance to it, result.summary() means and intervals over the draws.  One gradient pass where sobol needs
        Dx + 2 value passes.  Emulators of GP nodes only (ValueError)."""
        from . import sensitivity
        X = sensitivity.uniform_design(bounds, n_rows, seed, qmc)
        return self.sample_functions(sample_size, n_features).active_subspace(X, bounds)

    def thompson(self, bounds, batch_size=1, n_features=2048, maximize=False, output=0, **minimize_kw):
        """A batch of Thompson-sampling proposals for minimising (maximize: maximising) output `output` of the emulated
        function over the box bounds (Dx, 2) (optimize, DESIGN I.17): draws ceil(batch_size / N) functions per imputation
        (sample_functions, with its refusals), minimises every draw on the device (paths.minimize(bounds, **minimize_kw))
        and returns (X_new (batch_size, Dx), the optimize.PathOptimum of all draws): row b is the optimum of path
        (b mod N) * J + b div N, so a batch spreads over the imputations first."""
        from . import optimize
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError('thompson: batch_size must be at least 1')
        J = -(-batch_size // self.N)
        res = self.sample_functions(J, n_features).minimize(bounds, output=output, maximize=maximize, **minimize_kw)
        return optimize.thompson_rows(res, batch_size, self.N, J), res

    def calibrate(self, y, obs_sd, bounds, sample_size=10, n_features=2048, **calibrate_kw):
        """Bayesian calibration: the posterior of the input x over the box bounds (Dx, 2) given an observation y of the
        last layer's outputs with error sd obs_sd (calibrate, DESIGN I.19): draws sample_size functions per imputation
        (sample_functions, with its refusals), samples every draw's p(x | y, f) on the device (paths.calibrate(y, obs_sd,
        bounds, **calibrate_kw)) and returns the calibrate.PathPosterior of the N * sample_size draws; its pooled() samples
        are the modular posterior of x (Liu, Bayarri and Berger 2009)."""
        return self.sample_functions(sample_size, n_features).calibrate(y, obs_sd, bounds, **calibrate_kw)

    def calibrate_smc(self, y, obs_sd, bounds, sample_size=10, n_features=2048, **smc_kw):
        """calibrate by tempered sequential Monte Carlo (DESIGN I.21): draws sample_size functions per imputation and
        returns the calibrate.ParticlePosterior of paths.calibrate_smc(y, obs_sd, bounds, **smc_kw): every draw's
        particles and evidence; draw_weights() weighs the draws by it, pooled() is the modular posterior."""
        return self.sample_functions(sample_size, n_features).calibrate_smc(y, obs_sd, bounds, **smc_kw)

    def failure_probability(self, threshold, bounds, sample_size=10, n_features=2048, **sus_kw):
        """Draws sample_size functions (sample_functions(sample_size, n_features)) and returns the
        reliability.FailureProbability of paths.failure_probability(threshold, bounds, **sus_kw): every draw's probability
        that the output reaches threshold when x is distributed over the box, by subset simulation on the device (DESIGN
        I.22); the spread over the draws is the model's uncertainty about that probability."""
        return self.sample_functions(sample_size, n_features).failure_probability(threshold, bounds, **sus_kw)

    def sample_paths_vecchia(self, x, sample_size=50, full_layer=False, m=50):
        """sample_paths by the Vecchia factorisation of each node's joint predictive distribution (vpaths, DESIGN I.11):
        the same container and column layout, for dense and Vecchia emulators and any number of rows.  The rows of x are
        drawn in one order, the emulator's sampling generator's permutation(M), taken first; every GP node then draws each
        row given its m nearest training rows (the imputation's latents below layer 1) and earlier-drawn rows of the same
        path, with one standard_normal((N, sample_size, M)) block per GP node as sample_paths.  With m >= n + M - 1 this is
        sample_paths' dense joint.  A conditioning block that does not factor is retried with a jitter, then raises
        numpy.linalg.LinAlgError naming its layer, node and imputation."""
        from . import vpaths
        if self.shard or getattr(self, 'shard_points', False):
            raise NotImplementedError("sample_paths_vecchia with the imputations sharded over ranks would return partial "
                                      "draws; use emulator(..., shard=False)")
        vpaths.check_args(x, m)
        e, rng = self.engine, self._sample_rng
        M, S, J = len(x), self.N, int(sample_size)
        drawer = vpaths.Vecchia(m, rng.permutation(M))

        def draw(l, k, nd, xin):
            Z = e.tensor(rng.standard_normal((S, J, M)).reshape(S * J, M))
            omega = None if nd.rep is None else e.tensor(nd.W_diag)
            if l == 0:
                return drawer.draw_shared(e, paths.hyper(nd), xin, (e.tensor(nd._X()), omega),
                                          e.tensor(np.stack([self._ys(s, l, k) for s in range(S)])), Z, J,
                                          'layer 1, node %d (shared by every imputation)' % (k + 1))
            train = paths.PerGroup(lambda s: (e.tensor(self._train_in(s, l, nd, True)), omega))
            return drawer.draw_per_path(e, paths.hyper(nd), xin, train, paths.PerGroup(lambda s: e.tensor(self._ys(s, l, k))), Z,
                                        np.repeat(np.arange(S), J),
                                        lambda p: 'layer %d, node %d, imputation %d' % (l + 1, k + 1, p // J + 1))
        return self._walk_paths(x, J, full_layer, draw)

    def _walk_paths(self, x, J, full_layer, draw):
        """sample_paths' and sample_paths_vecchia's walk (pathwalk.walk over all_layer, the same structure for every
        imputation) and their container.  draw(l, k, nd, xin) -> (N*J, M) draws GP node k of layer l at xin, (M, D) in the
        first layer and (N*J, M, D) below it, and takes the node's normals from the generator."""
        e = self.engine
        xd = e.tensor(x)
        walk = pathwalk.walk(e, [self.all_layer] * self.N, J, xd, None, lambda nd: pathwalk.first(xd, nd),
                             lambda l, k, nodes, xin: draw(l, k, nodes[0], xin))
        out = [cur.cpu().numpy() for cur in walk]
        out = [list(a.transpose(2, 1, 0)) for a in out]
        return out if full_layer else out[-1]

    def _ys(self, s, l, k):
        """The training outputs of node k of layer l in imputation s: its latents, or the node's output in the last layer."""
        return self.latents[s][l][:, k] if l < self.n_layer - 1 else np.asarray(self.all_layer[l][k].output, float).reshape(-1)

    def _train_in(self, s, l, nd, with_global=False):
        """The training inputs of node nd of layer l > 0 in imputation s (host): its input_dim columns of the latents below,
        with_global followed by the node's global columns."""
        Xin = self.latents[s][l - 1][:, nd.input_dim]
        Xg = peek(nd, 'global_input') if with_global else None
        return Xin if Xg is None else np.concatenate((Xin, Xg), 1)

    def _joint_stats(self, l, k):
        """sample_paths' statistics of GP node k of layer l, built when first asked for beside predict's: L^-1 of the
        training correlation matrix (not the Matern cell reordering of the linked predictor: a permuted L^-1 is not
        triangular).  First layer: one L^-1 shared by every imputation, the N imputations' outputs as rows Y; deeper
        layers: L^-1 and y per imputation, through _LazyPer under the same byte budget."""
        if self._stats is None:
            self._build_stats()
        key = ('joint', l, k)
        st = self._stats.get(key)
        if st is not None:
            return st
        e = self.engine
        nd = self.all_layer[l][k]
        Xg = None if peek(nd, 'global_input') is None else e.tensor(peek(nd, 'global_input'))
        W = None if nd.rep is None else e.tensor(nd.W_diag)
        if l == 0:
            Linv = paths.factor_inverse(e, nd.name, e.tensor(peek(nd, 'input')), Xg, W, nd.length, nd.nugget[0],
                                        'layer 1, node %d (shared by every imputation)' % (k + 1))
            st = dict(Linv=Linv, W=e.tensor(nd._X()), Y=e.tensor(np.stack([self._ys(s, l, k) for s in range(self.N)])))
        else:
            def build(s):
                Linv = paths.factor_inverse(e, nd.name, e.tensor(self._train_in(s, l, nd)), Xg, W, nd.length, nd.nugget[0],
                                            'layer %d, node %d, imputation %d' % (l + 1, k + 1, s + 1))
                return dict(Linv=Linv, W=e.tensor(self._train_in(s, l, nd, True)), y=e.tensor(self._ys(s, l, k)))
            Np = e.padded_dim(len(nd.output))
            st = dict(per=_LazyPer(self, key, build, Np * Np * 8))
        self._stats[key] = st
        return st

    def nllik(self, x, y, m=50):
        """Negative predicted log-likelihood of test data under a DGP with ONE likelihood node on top
        (emulation.py:856-914): per imputation the latents' moments at x, the likelihood integrated by
        Gauss-Hermite quadrature (ghdiag), averaged over imputations.  Returns (mean, per-point values)."""
        from .likelihood_class import ghdiag
        if len(self.all_layer[-1]) != 1 or self.all_layer[-1][0].type != 'likelihood':
            raise Exception('The method is only applicable to a DGP with the final layer formed by only ONE node, which '
                            'must be a likelihood node.')
        if self.shard:
            raise NotImplementedError('nllik is evaluated on one rank (emulator(..., shard=False))')
        X0, indices = np.unique(x, return_inverse=True, axis=0)
        indices = np.asarray(indices).reshape(-1)
        if len(X0) != len(x):
            x = X0
        pm, pv = self._host_moments(x, m)[-2]
        lik = [ghdiag(self.all_layer[-1][0].pllik, pm[s][indices, :], pv[s][indices, :], y) for s in range(self.N)]
        nl = -np.log(np.mean(lik, axis=0)).flatten()
        return np.mean(nl), nl

    def _predict_points(self, x, method, full_layer, sample_size, m, aggregation):
        """shard='points': this rank predicts its block of rows of x with all N imputations; the blocks are gathered."""
        if method != 'mean_var' or not aggregation:
            raise NotImplementedError("shard='points' covers predict(method='mean_var') with aggregation")
        M = len(x)
        lo, hi = ddist.row_range(M, ddist.rank(), ddist.world())
        xs = x[lo:hi] if hi > lo else x[:1]         # (a rank without rows still takes part in the gather)
        self._in_points = True
        try:
            mu, var = self.predict(xs, method, full_layer, sample_size, m, True)
        finally:
            self._in_points = False
        dev = self.engine.device if ddist.td.get_backend() == 'nccl' else None
        g = lambda a: ddist.allgather_rows(a[:hi - lo], M, dev)
        if full_layer:
            return [g(a) for a in mu], [g(a) for a in var]
        return g(mu), g(var)

    def ppredict(self, x, method='mean_var', full_layer=False, sample_size=50, m=50, chunk_num=None, core_num=None):
        """emulation.py:578-629 split x over a process pool; test points and imputations already run in parallel on the
        device (`chunk_num` / `core_num` are accepted and unused)."""
        return self.predict(x, method=method, full_layer=full_layer, sample_size=sample_size, m=m)

    @contextlib.contextmanager
    def change_vecch_state(self):
        """Leave-one-out state of the Vecchia prediction branches (emulation.py:90-108): within the context every GP
        node drops the nearest of its conditioning points."""
        gps = [nd for layer in self.all_layer for nd in layer if nd.type == 'gp']
        for nd in gps:
            nd.loo_state = True
        try:
            yield
        finally:
            for nd in gps:
                nd.loo_state = False

    def loo(self, X, method=None, sample_size=50, m=30):
        """Leave-one-out cross validation at the training inputs X (emulation.py:109-143): every GP node conditions on
        its nearest training points with the nearest one (at the first layer the point itself) dropped
        (kernel_class.py:610-611,655-656) -- m of them for a Vecchia emulator, all other n-1 points for a dense one.
        The dense case does not run n factorisations of size n-1 as the reference does: it reuses the emulator's R^-1
        through the rank-one downdate of `_node_dense(loo=True)`."""
        if method is None:
            method = 'mean_var'
        per_layer, indices = self._loo_walk(X, m)
        res = self._draw_samples(_host(per_layer), sample_size, False) if method == 'sampling' else self._aggregate(per_layer)
        if indices is not None:
            res = type(res)(item[indices, :] for item in res)
        return res

    def _loo_walk(self, X, m):
        """loo's layer walk: the per-layer moments at the distinct rows of X, and for an X with replicated rows the index of
        each of its rows among them (else None)."""
        n_train = len(self.all_layer[0][0].input)
        indices = None
        if len(X) != n_train:
            X, indices = np.unique(X, return_inverse=True, axis=0)
            indices = np.asarray(indices).reshape(-1)
        if not self.vecch:
            return self._layer_moments(X, 'loo'), indices
        with self.change_vecch_state():
            return self._layer_moments(X, 'vecchia', m + 1), indices

    def _loo_moments(self, X, m):
        """_loo_walk's moments with the replicated rows put back: per layer (mean, var), (S, len(X), K) device tensors."""
        per_layer, indices = self._loo_walk(X, m)
        if indices is None:
            return per_layer
        idx = torch.as_tensor(indices, device=self.engine.device)
        return [(a[:, idx], b[:, idx]) for a, b in per_layer]

    def ploo(self, X, method=None, sample_size=50, m=30, core_num=None):
        """emulation.py:146-168 (`core_num` is accepted and unused)."""
        return self.loo(X, method=method, sample_size=sample_size, m=m)

    def metric(self, x_cand, method='ALM', obj=None, nugget_s=1., m=50, score_only=False):
        """Sequential-design criterion at the rows of x_cand (emulation.py:323-420).  ALM (the predictive variance)
        MICE and VIGF (GP hierarchies) are computed from the device layer walk."""
        if x_cand.ndim == 1:
            raise Exception('The candidate design set has to be a numpy 2d-array.')
        lik = any(nd.type == 'likelihood' for nd in self.all_layer[-1])
        L = self.n_layer - 2 if lik else self.n_layer - 1      # the last GP layer carries the criteria (emulation.py:347-420)
        if method == 'ALM':
            if lik:
                sigma2 = self.predict(x=x_cand, full_layer=True, m=m)[1][-2]
            else:
                _, sigma2 = self.predict(x=x_cand, m=m)
            if score_only:
                return sigma2
            idx = np.argmax(sigma2, axis=0)
            return idx, sigma2[idx, np.arange(sigma2.shape[1])]
        if method not in ('MICE', 'VIGF'):
            raise Exception("method must be 'ALM', 'MICE' or 'VIGF'.")
        if self.shard:
            raise NotImplementedError('MICE / VIGF are evaluated on one rank (emulator(..., shard=False))')
        if method == 'VIGF':
            return self._vigf(x_cand, obj, m, score_only)
        # MICE (emulation.py:377-394): mean over imputations of log(predictive variance / smoothed variance of a GP whose
        # design is the candidate set itself, functions.mice_var :244-256)
        per_layer = self._host_moments(x_cand, m)
        sigma2 = per_layer[L][1]
        pred_in = per_layer[L - 1][0] if L > 0 else None
        M, D, S = len(x_cand), len(self.all_layer[L]), self.N
        if lik and self.n_layer == 2:
            # one GP layer under a likelihood (emulation.py:366-375): its predictive variance does not depend on the
            # imputation; the ratio itself is the score
            s_0 = np.stack([_mice_var(self.engine, x_cand, x_cand, nd, nugget_s) for nd in self.all_layer[0]], 1)
            avg = sigma2[0] / s_0
        else:
            mice = np.zeros((M, D))
            for i in range(S):
                s_i = np.empty((M, D))
                for k, nd in enumerate(self.all_layer[L]):
                    s_i[:, k] = _mice_var(self.engine, x_cand if pred_in is None else pred_in[i], x_cand, nd, nugget_s)
                with np.errstate(divide='ignore'):
                    mice += np.log(sigma2[i] / s_i)
            avg = mice / S
        if score_only:
            return avg
        idx = np.argmax(avg, axis=0)
        return idx, avg[idx, np.arange(avg.shape[1])]

    def _vigf(self, x_cand, obj, m, score_only):
        """VIGF criterion (emulation.py:396-420, predict_vigf :526-576) for GP hierarchies: with b the squared
        difference between the imputation's predictive mean and the output at the nearest training input, and s2 its
        predictive variance, E[b^2 + 6 b s2 + 3 s2^2] - (E[b + s2])^2 over the imputations."""
        if obj is None:
            raise Exception('The dgp object that is used to build the emulator must be supplied to the argument `obj` '
                            'when VIGF criterion is chosen.')
        lik = any(nd.type != 'gp' for nd in self.all_layer[-1])
        if obj.indices is not None and not lik:
            raise Exception('VIGF criterion is currently not applicable to DGP emulators whose training data contain '
                            'replicates but without a likelihood node.')
        L = self.n_layer - 2 if lik else self.n_layer - 1
        X = obj.X
        e = self.engine
        if len(x_cand) * len(X) <= 20_000_000:
            d2 = (x_cand ** 2).sum(1)[:, None] - 2.0 * x_cand @ X.T + (X ** 2).sum(1)[None, :]
            index = np.argmin(d2, axis=1)
        else:
            index = e.nn_query(e.tensor(x_cand), e.tensor(X), 1).cpu().numpy().reshape(-1)
        mean, var = self._host_moments(x_cand, m)[L]
        if lik:    # under a likelihood the last GP layer's "outputs" are the imputation's own latents (emulation.py:498-524,567-570)
            Ytr = np.stack([self.latents[s_][L][index, :] for s_ in range(self.N)])                          # (S, M, D)
        else:
            Ytr = np.stack([np.asarray(nd.output, float).reshape(-1)[index] for nd in self.all_layer[-1]], 1)[None]   # (1, M, D)
        bias = (mean - Ytr) ** 2
        E1 = np.mean(bias ** 2 + 6 * bias * var + 3 * var ** 2, axis=0)
        E2 = np.mean(bias + var, axis=0)
        vigf = E1 - E2 ** 2
        if score_only:
            return vigf
        idx = np.argmax(vigf, axis=0)
        return idx, vigf[idx, np.arange(vigf.shape[1])]

    def pmetric(self, x_cand, method='ALM', obj=None, nugget_s=1., m=50, score_only=False, chunk_num=None, core_num=None):
        """emulation.py:170-321 (`chunk_num` / `core_num` are accepted and unused)."""
        return self.metric(x_cand, method=method, obj=obj, nugget_s=nugget_s, m=m, score_only=score_only)
