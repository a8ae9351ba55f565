"""Linked (D)GP emulation of a feed-forward system of emulators -- mirror of dgpsi.container / dgpsi.lgp
(linkgp.py:12-608), mean/variance prediction; joint sample paths of the system (lgp.sample_paths with the drawer
paths.Dense, lgp.sample_paths_vecchia with vpaths.Vecchia; DGP emulators walked by pathwalk.walk).  Pure orchestration
over kernel.gp_prediction / linkgp_prediction (GP emulators) and pathwalk.moments over kernel.predict_at / predict_link
(DGP emulators); aggregation over imputations as emulation.py:846-847."""
import collections
import contextlib
import copy

import numpy as np
import torch

from . import mixture, paths, pathwalk
from .imputation import imputer
from .kernel_class import peek


class container:
    """A trained GP (`gp.export()`) or DGP (`dgp.estimate()`) with its wiring into the system
    (linkgp.py:12-56).  local_input_idx: indices of the feeding layer's outputs (1d-array), or a list with one
    entry (array or None) per preceding layer."""

    def __init__(self, structure, local_input_idx=None, block=True):
        if len(structure) == 1:
            self.type, self.structure = 'gp', structure[0]
            self.vecch = bool(self.structure.vecch)
        else:
            self.type, self.structure = 'dgp', structure
            self.vecch = bool(structure[0][0].vecch)
            self.imp = imputer(self.structure, block)
            if self.vecch:
                self.imp.update_ord_nn()
            self.imp.sample(burnin=50)
        self.local_input_idx = local_input_idx

    def _gp_nodes(self):
        return [self.structure] if self.type == 'gp' else [nd for layer in self.structure for nd in layer if nd.type == 'gp']

    def to_vecchia(self):
        """Vecchia predictions for this emulator (linkgp.py:64-75)."""
        if not self.vecch:
            self.vecch = True
            for nd in self._gp_nodes():
                nd.vecch = True

    def remove_vecchia(self):
        """Dense predictions (linkgp.py:77-89); the n x n statistics are rebuilt on first use."""
        if self.vecch:
            self.vecch = False
            for nd in self._gp_nodes():
                nd.vecch = False
                nd._stats = None

    def set_local_input(self, idx, new=False):
        if not new:
            self.local_input_idx = idx
            return None
        c = copy.copy(self)
        c.local_input_idx = idx
        return c

    def __copy__(self):
        c = type(self).__new__(type(self))
        c.__dict__.update(self.__dict__)
        c.local_input_idx = copy.copy(self.local_input_idx)
        return c

    def _snapshot(self):
        """Copy holding the current imputation (arrays only; device statistics are rebuilt on first use)."""
        c = type(self).__new__(type(self))
        c.type, c.vecch, c.local_input_idx = self.type, self.vecch, copy.copy(self.local_input_idx)
        c.structure = copy.deepcopy(self.structure)
        nodes = [c.structure] if c.type == 'gp' else [nd for layer in c.structure for nd in layer]
        src = [self.structure] if self.type == 'gp' else [nd for layer in self.structure for nd in layer]
        for a, b in zip(nodes, src):
            if getattr(b, 'type', None) == 'gp':
                a.engine = b.engine
        return c


def _ensure_stats(nd):
    if nd.type == 'gp' and not nd.vecch and nd._stats is None:
        nd.compute_stats()


class _DenseTrain:
    """The training side of one GP node position for paths.Dense: lgp._node_stats' cached L^-1, W and y.  classes():
    cls[s] system s's training set among the distinct ones, call[s] what one device call holds fixed; shared(cs): (train, Y)
    of the systems cs, which share one training set; per_path(ss, J): (train, y, group) of the systems ss, J paths each."""

    def __init__(self, sysm, e, pos, nodes, where):
        self.stats = lambda: sysm._node_stats(e, pos, nodes, where)

    def classes(self):
        self.st = self.stats()
        return self.st['cls'], self.st['call']

    def _of(self, s):
        ps = self.st['per'][self.st['cls'][s]]
        return ps['W'], ps['Linv']

    def shared(self, cs):
        return self._of(cs[0]), torch.stack([self.st['y'][s] for s in cs])

    def per_path(self, ss, J):
        return (paths.PerGroup(lambda i: self._of(ss[i])), paths.PerGroup(lambda i: self.st['y'][ss[i]]),
                np.repeat(np.arange(len(ss)), J))


class _VecchiaTrain:
    """The same for vpaths.Vecchia: nothing cached, tensors made when a chunk asks for them.  One call also holds one set of
    replicate weights (omega); systems that share training inputs and outputs by content (the copies of a GP emulator)
    need no group."""

    def __init__(self, e, nodes):
        self.e, self.nodes = e, nodes

    def classes(self):
        self.cls, call, _ = lgp._node_classes(self.nodes)
        return self.cls, [(c, None if nd.rep is None else np.asarray(nd.W_diag, float).tobytes())
                          for c, nd in zip(call, self.nodes)]

    def _in(self, s):
        return self.e.tensor(np.ascontiguousarray(self.nodes[s]._X(), dtype=float))

    def _out(self, s):
        return np.asarray(self.nodes[s].output, dtype=float).reshape(-1)

    def _omega(self, s):
        return None if self.nodes[s].rep is None else self.e.tensor(self.nodes[s].W_diag)

    def shared(self, cs):
        return (self._in(cs[0]), self._omega(cs[0])), self.e.tensor(np.stack([self._out(s) for s in cs]))

    def per_path(self, ss, J):
        omega = self._omega(ss[0])
        W0 = self._in(ss[0]) if len({self.cls[s] for s in ss}) == 1 else None
        if W0 is not None and all(np.array_equal(self._out(ss[0]), self._out(s)) for s in ss[1:]):
            return (W0, omega), self.e.tensor(self._out(ss[0])), None
        return (paths.PerGroup(lambda g: (self._in(ss[g]) if W0 is None else W0, omega)),
                paths.PerGroup(lambda g: self.e.tensor(self._out(ss[g]))), np.repeat(np.arange(len(ss)), J))


class lgp:
    """all_layer: list of layers of containers; N imputations (1 if the system has GP emulators only)  (linkgp.py:140-165).
    `sample_paths` draws whole functions of the system (dense emulators, at most 8192 rows): column s*sample_size + j is one
    joint draw over all rows of x, the same path in every emulator and layer.  `sample_paths_vecchia` draws the same paths
    from each GP node's m nearest training and earlier-drawn rows: dense and Vecchia-mode emulators in any mixture, any
    number of rows, cost linear in the rows."""

    def __init__(self, all_layer, N=10):
        self.L = len(all_layer)
        self.all_layer = all_layer
        self.num_model = [len(layer) for layer in all_layer[1:]]
        if not any(c.type == 'dgp' for layer in all_layer for c in layer):
            N = 1
        self.all_layer_set = []
        for _ in range(N):
            one = []
            for layer in all_layer:
                row = []
                for c in layer:
                    if c.type == 'dgp':
                        if c.vecch:
                            c.imp.update_ord_nn()
                        c.imp.sample()
                    row.append(c._snapshot())
                one.append(row)
            self.all_layer_set.append(one)

    def set_vecchia(self, mode):
        """Vecchia (True) or dense (False) predictions for all emulators of the system, or per emulator with a list
        shaped like all_layer (linkgp.py:180-212)."""
        if isinstance(mode, list):
            if len(mode) != len(self.all_layer) or any(len(a) != len(b) for a, b in zip(mode, self.all_layer)):
                raise Exception('mode has a different shape as all_layer.')
        else:
            mode = [[mode for _ in layer] for layer in self.all_layer]
        for system in [self.all_layer] + list(self.all_layer_set):
            for layer, ml in zip(system, mode):
                for c, on in zip(layer, ml):
                    c.to_vecchia() if on else c.remove_vecchia()
        for a in ('_paths_stats', '_per_cache', '_per_bytes'):   # sample_paths' statistics are rebuilt on next use
            self.__dict__.pop(a, None)

    # -------------------------------------------------------------- single emulators
    @staticmethod
    def gp_pred(x, m, v, z, structure, m_pred):
        """GP emulator with deterministic (x) or Gaussian (m, v) inputs (linkgp.py:503-515)."""
        structure.pred_m = m_pred
        _ensure_stats(structure)
        if x is None:
            mu, s2 = structure.linkgp_prediction(m=m, v=v, z=z)
        else:
            mu, s2 = structure.gp_prediction(x=x, z=z)
        return mu.reshape(-1, 1), s2.reshape(-1, 1)

    @staticmethod
    def dgp_pred(x, m, v, z, structure, pred_m):
        """Layer walk through a DGP emulator whose input is deterministic (x) or Gaussian (m, v [+ external z])
        (linkgp.py:517-608, GP nodes).  Returns (mean, var) of the layer before last and of the last layer."""
        if pathwalk.is_categorical(structure[-1]):   # (the walk would hand back the feeding latents' moments)
            raise NotImplementedError('lgp: a DGP emulator with a Categorical likelihood on top cannot feed or end a linked system')
        e = structure[0][0].engine
        t = lambda a: None if a is None else e.tensor(np.asarray(a, float))
        if x is not None:   # (the first layer takes every column of x and z, and of m and z)
            m, first = x, pathwalk.Inputs(t(x if z is None else np.concatenate((x, z), 1)), None, None)
        else:
            first = pathwalk.Inputs(t(m), t(v), t(z))

        def node(il, j, nodes, inp):
            nd = nodes[0]
            nd.pred_m = pred_m
            _ensure_stats(nd)
            if inp.v is None:
                mk, vk = nd.predict_at(inp.m)
            elif il == 0:
                mk, vk = nd.predict_link(inp.m, inp.v, inp.z)
            else:   # (its global inputs may themselves be uncertain -- outputs of feeding emulators -- and / or external)
                mk, vk = nd.predict_link(inp.m[0], inp.v[0], inp.z)
            return mk[None], vk[None]
        out = [(a[0].cpu().numpy(), b[0].cpu().numpy())
               for a, b in pathwalk.moments(e, [structure], t(m), first.v, first.z, lambda nd: first, node)]
        return out[-2] + out[-1]

    def _emulate(self, model, x, m, v, z, pred_m, before=False):
        if model.type == 'gp':
            out = self.gp_pred(x, m, v, z, model.structure, pred_m)
            return (None, None) + out if before else out
        out = self.dgp_pred(x, m, v, z, model.structure, pred_m)
        return out if before else out[2:]

    @staticmethod
    def _draw(model, mk, vk, m_before, v_before, sample_size):
        """sample_size draws per test point from one emulator's predictive distributions, (q, M, sample_size)
        (linkgp.py:383-386,408-421).  A likelihood node on top of a DGP emulator samples y from draws of its feeding
        latents.  (For the GP nodes of a DGP emulator in the last layer the reference takes the spread from the layer
        before, linkgp.py:416 -- a slip that fails as soon as the two layers differ in width; the nodes' own
        predictive variances are used here.)"""
        M, q = mk.shape
        if model.type == 'gp' or all(nd.type == 'gp' for nd in model.structure[-1]):
            return np.random.normal(mk, np.sqrt(vk), size=(sample_size, M, q)).transpose(2, 1, 0)
        out = np.empty((q, M, sample_size))
        for c, nd in enumerate(model.structure[-1]):
            if nd.type == 'gp':
                out[c] = np.random.normal(mk[:, [c]], np.sqrt(vk[:, [c]]), size=(M, sample_size))
            else:
                lat = np.random.normal(m_before, np.sqrt(v_before), size=(sample_size,) + m_before.shape)
                out[c] = np.array([nd.sampling(lat[i][:, nd.input_dim]) for i in range(sample_size)]).T
        return out

    # -------------------------------------------------------------- the system
    def _global_inputs(self, x):
        """x as the per-layer list of global inputs (predict's forms and checks)."""
        if isinstance(x, list):
            if len(x) != self.L:
                raise Exception('When test input is given as a list, it must contain global inputs to the all layers '
                                '(even with no global inputs to internal layers). Set None as the global input to the '
                                'internal models if they have no global inputs.')
            return x
        if x.ndim == 1:
            raise Exception('The testing input has to be a numpy 2d-array.')
        return [x] + [[None] * k for k in self.num_model]

    @staticmethod
    def _feeding(model, l):
        """local_input_idx of an emulator in layer l > 0 as a list over the layers before it (entries None or columns)."""
        idx = model.local_input_idx
        if l == 0:
            if isinstance(idx, list):
                raise Exception('When an emulator is in the first layer, local_input_idx must be a 1d-array.')
            return idx
        if not isinstance(idx, list):
            return [None] * (l - 1) + [idx]
        if len(idx) != l:
            raise Exception('local_input_idx should be a list that has length of %i.' % l)
        return idx

    def _system_moments(self, x, m, full_layer=False, sample_size=None):
        """The walk through every system (imputation) of the set: per system the (M x q) means and variances of the final
        layer's emulators -- of every layer's with full_layer -- and with a sample_size the draws from them (else empty
        lists).  predict aggregates these; predict_dist keeps them as the components of the mixtures."""
        sampling = sample_size is not None
        x = self._global_inputs(x)
        means, variances, draws = [], [], []
        for one in self.all_layer_set:
            feed_m, feed_v, lay_m, lay_v, lay_s = [], [], [], [], []
            for l, layer in enumerate(one):
                ms, vs, ss = [], [], []
                for k, model in enumerate(layer):
                    if l == 0:
                        self._feeding(model, l)
                        mb, vb, mk, vk = self._emulate(model, x[0][:, model.local_input_idx], None, None, None, m, before=True)
                    else:
                        idx = self._feeding(model, l)
                        m_in = np.concatenate([feed_m[i][:, j] for i, j in enumerate(idx) if j is not None], axis=1)
                        v_in = np.concatenate([feed_v[i][:, j] for i, j in enumerate(idx) if j is not None], axis=1)
                        mb, vb, mk, vk = self._emulate(model, None, m_in, v_in, x[l][k], m, before=True)
                    ms.append(mk)
                    vs.append(vk)
                    if sampling and (full_layer or l == self.L - 1):
                        ss.append(self._draw(model, mk, vk, mb, vb, sample_size))
                lay_m.append(ms)
                lay_v.append(vs)
                lay_s.append(ss)
                feed_m.append(np.concatenate(ms, axis=1))
                feed_v.append(np.concatenate(vs, axis=1))
            means.append(lay_m if full_layer else lay_m[-1])
            variances.append(lay_v if full_layer else lay_v[-1])
            draws.append(lay_s if full_layer else lay_s[-1])
        return means, variances, draws

    def predict(self, x, method='mean_var', full_layer=False, sample_size=50, m=50):
        """Means and variances of the final-layer emulators' outputs (lists of (M x q) arrays), or of every
        layer if full_layer (linkgp.py:285-501); method='sampling': per emulator an array (q, M, N * sample_size) of
        draws from the imputations' predictive distributions."""
        if method not in ('mean_var', 'sampling'):
            raise Exception("method must be either 'mean_var' or 'sampling'.")
        sampling = method == 'sampling'
        means, variances, draws = self._system_moments(x, m, full_layer, sample_size if sampling else None)
        if sampling:    # per emulator (q, M, S * sample_size): the imputations' draws side by side (linkgp.py:496-500)
            if full_layer:
                return [[np.concatenate([draws[s_][l][k] for s_ in range(len(draws))], axis=2)
                         for k in range(len(self.all_layer[l]))] for l in range(self.L)]
            return [np.concatenate([draws[s_][k] for s_ in range(len(draws))], axis=2) for k in range(len(self.all_layer[-1]))]

        agg = mixture.host_moments   # emulation.py:846-847 over the imputations
        if full_layer:
            out = [[agg([means[s][l][k] for s in range(len(means))], [variances[s][l][k] for s in range(len(means))])
                    for k in range(len(self.all_layer[l]))] for l in range(self.L)]
            return [[o[0] for o in row] for row in out], [[o[1] for o in row] for row in out]
        out = [agg([means[s][k] for s in range(len(means))], [variances[s][k] for s in range(len(means))])
               for k in range(len(self.all_layer[-1]))]
        return [o[0] for o in out], [o[1] for o in out]

    def predict_dist(self, x, m=50):
        """The predictive distributions of the final-layer emulators' outputs at the rows of x: a list over those emulators of
        mixture.PredictiveMixture, each the equal-weight mixture of the N systems' Gaussians (M points x q outputs) -- mean()
        and var() are predict(x)'s; cdf, sf, logpdf, quantile, interval and crps are evaluated on the device (DESIGN I.15).
        A final emulator that ends in a likelihood node raises ValueError: its predictive distribution is no mixture of
        Gaussians (draw from it with predict(method='sampling'))."""
        for c in self.all_layer[-1]:
            if c.type == 'dgp' and any(nd.type == 'likelihood' for nd in c.structure[-1]):
                raise ValueError('predict_dist: with a likelihood node on top of a final emulator the predictive distribution is '
                                 "not a mixture of Gaussians; draw from it with predict(method='sampling')")
        means, variances, _ = self._system_moments(x, m)
        out = []
        for k, c in enumerate(self.all_layer_set[0][-1]):
            e = (c.structure if c.type == 'gp' else c.structure[0][0]).engine
            out.append(mixture.PredictiveMixture(e, e.tensor(np.stack([ms[k] for ms in means])),
                                                 e.tensor(np.stack([vs[k] for vs in variances])), host_moments=True))
        return out

    # -------------------------------------------------------------- joint sample paths
    def sample_paths(self, x, sample_size=50, full_layer=False):
        """Joint draws of the system's functions at the rows of x (dense emulators).  x as in predict.  Returns the layout of
        predict(x, method='sampling'): per final-layer emulator a (q, M, N*sample_size) array, or with full_layer a list
        over layers of such lists -- but column s*sample_size + j is ONE draw over all M rows: path j of system s
        (all_layer_set[s]), the same path in every emulator and layer.  Each path walks the system layer by layer, emulator
        by emulator, and within a DGP emulator layer by layer and node by node: a GP node is drawn jointly from its
        posterior at the path's inputs -- the feeding emulators' draws of this path selected by local_input_idx, plus
        x[l][k]; a DGP node with `connect` takes its global columns as predict does (the path's draws of the emulator's own
        inputs, external ones from x[l][k]); likelihood nodes sample from the path's latents (nd.sampling, or the class
        probabilities of a Categorical node).  Normals come from numpy's global generator: one
        np.random.standard_normal((N, sample_size, M)) block per GP node in that walk order; likelihood nodes sample after
        the GP nodes of their layer.  At most 8192 rows (ValueError); a Vecchia emulator raises NotImplementedError and a
        training correlation matrix that is not positive definite numpy.linalg.LinAlgError, naming where."""
        x = self._global_inputs(x)
        idxs = [[self._feeding(c, l) for c in layer] for l, layer in enumerate(self.all_layer)]
        for system in [self.all_layer] + list(self.all_layer_set):
            for l, layer in enumerate(system):
                for k, c in enumerate(layer):
                    if c.vecch:
                        raise NotImplementedError('sample_paths needs dense emulators: emulator %d of layer %d is in Vecchia '
                                                  'mode (joint draws of a Vecchia emulator need a sparse algorithm of their '
                                                  'own; use sample_paths_vecchia, or set_vecchia(False))' % (k + 1, l + 1))
        paths.check_points(x[0])
        J = int(sample_size)

        def draw(e, pos, nodes, xin, where):
            where += ' (gp)' if len(pos) == 2 else ''
            return self._paths_node(e, nodes, xin, J, paths.Dense(), _DenseTrain(self, e, pos, nodes, where), where)
        return self._paths_walk(x, idxs, J, full_layer, draw)

    def sample_paths_vecchia(self, x, sample_size=50, full_layer=False, m=50):
        """sample_paths by the Vecchia factorisation of every GP node's joint predictive distribution (vpaths, DESIGN I.11):
        the same walk, container and column layout, for any mixture of dense and Vecchia-mode emulators (the draw never
        reads the n x n statistics) and any number of rows.  The rows of x are drawn in one order,
        np.random.permutation(M), taken first and used by every emulator, layer, node and path; every GP node then draws
        each row given the min(m, n + i) nearest of its n training rows (nd._X() and nd.output: a system's own latents
        below the first layer of a DGP emulator) and of the same path's rows drawn before it, with one
        np.random.standard_normal((N, sample_size, M)) block per GP node in walk order, indexed by the rows of x; likelihood
        nodes sample after the GP nodes of their layer.  A system of one GP container returns gp.sample_paths_vecchia's
        draws; with m >= n + M - 1 at every node the paths have sample_paths' distribution.  Nodes whose inputs every
        path shares (layer 1 of the system) take one neighbour search for all paths (Vecchia.draw_shared); every other
        node draws all systems in one call per chunk of paths (Vecchia.draw_per_path), split only where the systems' nodes
        differ in kernel, hyper-parameters, training-set shape or replicate weights.  Nothing is kept across calls.
        m < 1 raises ValueError; a conditioning block that does not factor is retried with a jitter, then raises
        numpy.linalg.LinAlgError naming layer, emulator, node and system."""
        from . import vpaths
        x = self._global_inputs(x)
        idxs = [[self._feeding(c, l) for c in layer] for l, layer in enumerate(self.all_layer)]
        vpaths.check_args(x[0], m)
        J = int(sample_size)
        drawer = vpaths.Vecchia(m, np.random.permutation(len(x[0])))

        def draw(e, pos, nodes, xin, where):
            return self._paths_node(e, nodes, xin, J, drawer, _VecchiaTrain(e, nodes), where)
        return self._paths_walk(x, idxs, J, full_layer, draw)

    def _paths_walk(self, x, idxs, J, full_layer, draw):
        """The walk of sample_paths and sample_paths_vecchia: layer by layer and emulator by emulator, every path fed its
        own draws of the emulators before it.  draw(e, pos, nodes, xin, where) -> (S*J, M) draws one GP node over all
        systems (pos its place: (l, k) for a GP emulator, (l, k, il, j) inside a DGP emulator; nodes[s] system s's node; xin
        (M, D) shared by every path or (S*J, M, D)) and takes the node's normals from numpy's global generator."""
        sets = self.all_layer_set
        e = next(c.structure.engine if c.type == 'gp' else c.structure[0][0].engine for c in sets[0][0])
        M = len(x[0])
        feed, out = [], []
        for l in range(self.L):
            outs = []
            for k in range(len(self.all_layer[l])):
                models = [one[l][k] for one in sets]
                z = None if l == 0 or x[l][k] is None else e.tensor(np.asarray(x[l][k], float))
                if l == 0:   # the same inputs for every path
                    m = e.tensor(np.ascontiguousarray(x[0][:, idxs[0][k]], dtype=float))
                else:
                    m = torch.cat([feed[i][:, :, torch.as_tensor(np.atleast_1d(j), device=e.device)]
                                   for i, j in enumerate(idxs[l][k]) if j is not None], 2)
                where = 'layer %d, emulator %d' % (l + 1, k + 1)
                if models[0].type == 'gp':
                    xin = m if z is None else torch.cat((m, z[None].expand(m.shape[0], M, z.shape[1])), 2)
                    cur = draw(e, (l, k), [c.structure for c in models], xin.contiguous(), where)[:, :, None]
                else:   # (its first layer takes every column of m and z)
                    xin = m if z is None else torch.cat([pathwalk.per_path(t, len(sets) * J) for t in (m, z)], 2)
                    for cur in pathwalk.walk(e, [c.structure for c in models], J, m, z, lambda nd: xin,
                                             lambda il, j, nodes, xi: draw(e, (l, k, il, j), nodes, xi, '%s, node %d of its '
                                                                           'layer %d' % (where, j + 1, il + 1))):
                        pass   # (the last layer's paths are the emulator's)
                outs.append(cur)
            feed.append(torch.cat(outs, 2))
            if full_layer or l == self.L - 1:
                out.append([c.permute(2, 1, 0).contiguous().cpu().numpy() for c in outs])
        return out if full_layer else out[-1]

    def _paths_node(self, e, nodes, xin, J, drawer, train, where):
        """Paths (S*J, M) of one GP node over all systems: nodes[s] is system s's node, xin its inputs, (M, D) shared by
        every path or (S*J, M, D); drawer paths.Dense or vpaths.Vecchia, train its _DenseTrain / _VecchiaTrain.  Draws this
        node's (S, J, M) block of normals.  Systems that one device call can hold (train.classes' call) draw together:
        through drawer.draw_shared for shared inputs, once per distinct training set with the systems' outputs as the rows
        of Y (an error names the first of them); else through drawer.draw_per_path with the system as each path's group."""
        S, M = len(nodes), xin.shape[-2]
        Z = np.random.standard_normal((S, J, M))
        cls, call = train.classes()
        calls = collections.defaultdict(list)
        for s in range(S):
            calls[call[s]].append(s)
        draws = []   # (systems, (len(systems)*J, M) paths)
        for ss in calls.values():
            hyper = paths.hyper(nodes[ss[0]])
            if xin.dim() == 2:
                by = collections.defaultdict(list)
                for s in ss:
                    by[cls[s]].append(s)
                for cs in by.values():
                    draws.append((cs, drawer.draw_shared(e, hyper, xin, *train.shared(cs), e.tensor(Z[cs].reshape(len(cs) * J, M)),
                                                         J, '%s, system %d' % (where, cs[0] + 1))))
                continue
            xs = xin if len(ss) == S else xin.view(S, J, M, -1)[torch.as_tensor(ss, device=e.device)].reshape(-1, M, xin.shape[2])
            tr, y, group = train.per_path(ss, J)
            draws.append((ss, drawer.draw_per_path(e, hyper, xs.contiguous(), tr, y, e.tensor(Z[ss].reshape(len(ss) * J, M)), group,
                                                   lambda p, ss=ss: '%s, system %d' % (where, ss[p // J] + 1))))
        if len(draws) == 1:
            return draws[0][1].contiguous()
        out = e.empty(S, J, M)
        for ss, o in draws:
            out[torch.as_tensor(ss, device=e.device)] = o.reshape(len(ss), J, M)
        return out.reshape(S * J, M)

    @staticmethod
    def _node_classes(nodes):
        """One GP node position over the systems, compared by content: cls[s] the index of system s's training set among
        the distinct ones (inputs, global inputs, replicate weights, lengths, nugget), first[c] the first system of set c,
        call[s] what one device call holds fixed (kernel, lengths, scale, nugget, training-set shape)."""
        cls, call, first, held, seen = [], [], [], [], {}
        for s, nd in enumerate(nodes):
            X, Xg = peek(nd, 'input'), peek(nd, 'global_input')
            big = [None if a is None else np.asarray(a, dtype=float) for a in (X, Xg, None if nd.rep is None else nd.W_diag)]
            length = np.asarray(nd.length, float).tobytes()
            # (shapes and sums only pick the candidates; equality of every element decides)
            key = (nd.name, length, np.asarray(nd.nugget, float).tobytes()) + \
                tuple(None if a is None else (a.shape, float(a.sum())) for a in big)
            for c in seen.setdefault(key, []):
                if all(a is None or np.array_equal(a, b) for a, b in zip(big, held[c])):
                    break
            else:
                c = len(first)
                seen[key].append(c)
                first.append(s)
                held.append(big)
            cls.append(c)
            call.append((nd.name, length, float(nd.scale[0]), float(nd.nugget[0]),
                         (np.shape(X)[0], np.shape(X)[1] + (0 if Xg is None else np.shape(Xg)[1]))))
        return cls, call, first

    def _node_stats(self, e, pos, nodes, where):
        """sample_paths' statistics of one GP node position over the systems, cached on the lgp (dropped by set_vecchia):
        y per system; L^-1 (paths.factor_inverse) and W per distinct training set -- inputs, replicate weights, lengths and
        nugget compared by content, so copies of one GP (lgp.__init__'s snapshots, or systems built by hand) and the
        first-layer nodes of a DGP emulator share one.  One distinct set is kept; several (the deeper nodes of a DGP
        emulator: one per system) are built when first asked for and kept under the emulator's byte budget (_LazyPer)."""
        from .emulation import _LazyPer
        cache = self.__dict__.setdefault('_paths_stats', {})
        st = cache.get(pos)
        if st is not None:
            return st
        self.__dict__.setdefault('_per_cache', collections.OrderedDict())
        self.__dict__.setdefault('_per_bytes', 0)
        cls, call, first = self._node_classes(nodes)

        def build(c):
            nd, s = nodes[first[c]], first[c]
            Xg = peek(nd, 'global_input')
            Linv = paths.factor_inverse(e, nd.name, e.tensor(np.ascontiguousarray(peek(nd, 'input'), dtype=float)),
                                        None if Xg is None else e.tensor(Xg), None if nd.rep is None else e.tensor(nd.W_diag),
                                        nd.length, nd.nugget[0], '%s, system %d' % (where, s + 1))
            return dict(Linv=Linv, W=e.tensor(np.ascontiguousarray(nd._X(), dtype=float)))

        if len(first) == 1:
            per = [build(0)]
        else:
            Np = e.padded_dim(len(nodes[0].output))
            per = _LazyPer(self, ('paths',) + tuple(pos), build, Np * Np * 8)
        st = dict(cls=cls, call=call, per=per,
                  y=[e.tensor(np.asarray(nd.output, dtype=float).reshape(-1)) for nd in nodes])
        cache[pos] = st
        return st

    @contextlib.contextmanager
    def temp_all_layer(self):
        """A deep copy of the linked structure to work on (linkgp.py:172-178)."""
        yield copy.deepcopy(self.all_layer)

    def ppredict(self, x, method='mean_var', full_layer=False, sample_size=50, m=50, chunk_num=None, core_num=None):
        """linkgp.py:214-262 (`chunk_num` / `core_num` are accepted and unused)."""
        return self.predict(x, method=method, full_layer=full_layer, sample_size=sample_size, m=m)
