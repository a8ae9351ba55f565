"""The two walks through one DGP hierarchy.  `walk`: joint sample paths, shared by emulator.sample_paths,
emulator.sample_paths_vecchia and the DGP emulators of an lgp (lgp.sample_paths, lgp.sample_paths_vecchia).  `moments`:
predictive means and variances, shared by emulator.predict / loo / metric / nllik (dense, leave-one-out and Vecchia) and
lgp.dgp_pred.  A walk assembles every node's inputs and lets likelihood nodes sample or predict; what a GP node does with
its inputs (statistics, drawer, generator) is the caller's `draw` / `node`."""
import collections

import numpy as np
import torch


def connect_split(connect, last, D, internal, external):
    """A node's `connect` columns, read against the emulator's own D input columns followed by its external ones
    (linkgp.py:538-560): i1 the columns of the input, i2 those of the external input.  The last layer's `connect` holds
    columns of the training input and is matched against the first layer's input_dim / connect (internal / external)."""
    if last:
        i1 = np.where(connect[:, None] == internal[None, :])[1]
        i2 = np.array([], dtype=int) if external is None else np.where(connect[:, None] == external[None, :])[1]
        return i1, i2
    return connect[connect <= D - 1], connect[connect > D - 1] - D


def cols(t, idx):
    """t[..., idx] of a device tensor for host indices."""
    return t[..., torch.as_tensor(idx, device=t.device)]


def first(xd, nd):
    """The input of first-layer node nd at the rows xd of the hierarchy's input, (M, Dx) or per path (P, M, Dx): its input_dim,
    then its connect columns."""
    xin = cols(xd, nd.input_dim)
    return xin if nd.connect is None else torch.cat((xin, cols(xd, nd.connect)), -1)


def per_path(t, P):
    """(M, D) shared by every path as (P, M, D); a (P, M, D) tensor as it is."""
    return t if t.dim() == 3 else t[None].expand(P, *t.shape)


def is_categorical(layer):
    return len(layer) == 1 and getattr(layer[0], 'name', None) == 'Categorical'


def connect_cols(nd, last, shared, D, head):
    """Where a deeper node's `connect` columns are read: (columns of the hierarchy's input, columns of its external input).
    shared: the input is deterministic, the same for every path and imputation, and `connect` indexes it as it stands;
    else it is split over the two by connect_split, against the input_dim / connect of `head`, the hierarchy's first node."""
    none = np.array([], dtype=int)
    if nd.connect is None:
        return none, none
    if shared:
        return np.asarray(nd.connect), none
    return connect_split(nd.connect, last, D, head.input_dim, head.connect)


def walk(e, structs, J, m, z, first, draw, own_input=False):
    """Paths of a DGP hierarchy, layer by layer: yields each layer's (P, M, K) device tensor, P = len(structs) * J, the
    last one the hierarchy's output (a Categorical top: its class probabilities).  structs[s] is the structure behind paths
    s*J .. (s+1)*J - 1 (an emulator: its all_layer for every imputation; an lgp: system s's snapshot); m the hierarchy's
    input, (M, D) shared by every path or (P, M, D); z its external input (M, Dz) or None; first(nd) the input of
    first-layer node nd, (M, D') or (P, M, D').  A deeper node sees its input_dim columns of the layer below plus its
    `connect` columns: of m when every path shares it, else split over m and z as lgp.dgp_pred does.  own_input: a per-path
    m (P, M, D) is the hierarchy's own input all the same (every path at rows of its own: PathFunctions.minimize), and
    `connect` indexes it as it stands, as it does a shared one.
    draw(il, j, nodes, xin) -> (P, M) draws GP node j of layer il (nodes[s] = structs[s][il][j]) at xin; likelihood nodes
    sample from the path's latents after the GP nodes of their layer (structs[p // J]'s node for path p)."""
    S, L = len(structs), len(structs[0])
    P, M = S * J, m.shape[-2]
    prev = None
    for il, layer in enumerate(structs[0]):
        if il == L - 1 and is_categorical(layer):
            cat, lat = layer[0], prev.cpu().numpy()
            yield e.tensor(np.stack([structs[p // J][il][0].sampling(lat[p][:, cat.input_dim]) for p in range(P)])
                           .reshape(P, M, -1))
            return
        cur = e.empty(P, M, len(layer))
        for j, nd in enumerate(layer):
            if nd.type != 'gp':
                continue
            if il == 0:
                xin = first(nd)
            else:
                own, ext = connect_cols(nd, il == L - 1, m.dim() == 2 or own_input, m.shape[-1], structs[0][0][0])
                xin = torch.cat([cols(prev, nd.input_dim)] + [per_path(cols(t, i), P) for t, i in ((m, own), (z, ext)) if i.size], 2)
            cur[:, :, j] = draw(il, j, [st[il][j] for st in structs], xin.contiguous())
        if any(nd.type != 'gp' for nd in layer):   # likelihood nodes sample y from the path's latents (emulation.py:785-822)
            cur_np, lat = cur.cpu().numpy(), prev.cpu().numpy()
            for j, nd in enumerate(layer):
                if nd.type != 'gp':
                    for p in range(P):
                        cur_np[p, :, j] = structs[p // J][il][j].sampling(lat[p][:, nd.input_dim])
            cur = e.tensor(cur_np)
        yield cur
        prev = cur


Inputs = collections.namedtuple('Inputs', 'm v z')
Inputs.__doc__ = """What a GP node predicts at: m its inputs -- deterministic (v None; global columns appended) or Gaussian
with variances v; z the deterministic global columns beside Gaussian ones, or None.  The first layer's are what `first`
returns; below it m and v are (S, M, D), z (M, Dz)."""


def moments(e, structs, m, v, z, first, node):
    """Predictive moments of a DGP hierarchy, layer by layer: yields each layer's (mean, var), device tensors (S, M, K),
    S = len(structs) (an emulator: its all_layer for every imputation; lgp.dgp_pred: the one structure).  A Categorical top
    yields its feeding columns of the layer below (they are aggregated first and turned into class probabilities after).
    m (M, D) is the hierarchy's input: deterministic if v is None, else Gaussian with variances v and external input z
    (M, Dz) or None.  first(nd) -> Inputs of first-layer node nd.  A deeper node sees, as Gaussian inputs, its input_dim
    columns of the layer below and, as global ones, its `connect` columns: of m when that is deterministic, else split over
    m (uncertain: they join the Gaussian inputs, after the local ones) and z as connect_cols says.
    node(il, j, nodes, inputs) -> (mean (S, M), var (S, M) or (M,)) predicts GP node j of layer il (nodes[s] =
    structs[s][il][j]); likelihood nodes take nd.prediction(m=, v=) of their feeding columns on the host after the GP nodes
    of their layer (emulation.py:738-770)."""
    S, L = len(structs), len(structs[0])
    M = m.shape[0]
    prev = None
    for il, layer in enumerate(structs[0]):
        if il == L - 1 and is_categorical(layer):
            yield tuple(cols(t, np.asarray(layer[0].input_dim)).contiguous() for t in prev)
            return
        mean, var = e.empty(S, M, len(layer)), e.empty(S, M, len(layer))
        for j, nd in enumerate(layer):
            if nd.type != 'gp':
                continue
            if il == 0:
                inp = first(nd)
            else:
                own, ext = connect_cols(nd, il == L - 1, v is None, m.shape[1], structs[0][0][0])
                pm, pv = (cols(t, nd.input_dim) for t in prev)
                if v is None:
                    inp = Inputs(pm.contiguous(), pv.contiguous(), cols(m, own).contiguous() if own.size else None)
                else:
                    if own.size:
                        pm, pv = (torch.cat((a, per_path(cols(b, own), S)), 2) for a, b in ((pm, m), (pv, v)))
                    inp = Inputs(pm.contiguous(), pv.contiguous(), cols(z, ext).contiguous() if ext.size else None)
            mean[:, :, j], var[:, :, j] = node(il, j, [st[il][j] for st in structs], inp)
        if any(nd.type != 'gp' for nd in layer):
            pm, pv = (t.cpu().numpy() for t in prev)
            for j, nd in enumerate(layer):
                if nd.type != 'gp':
                    for s in range(S):
                        mk, vk = structs[s][il][j].prediction(m=pm[s][:, nd.input_dim], v=pv[s][:, nd.input_dim])
                        mean[s, :, j], var[s, :, j] = e.tensor(mk), e.tensor(vk)
        yield mean, var
        prev = mean, var
