"""The walk of joint sample paths through one DGP hierarchy, shared by emulator.sample_paths, emulator.sample_paths_vecchia
and the DGP emulators of an lgp (lgp.sample_paths, lgp.sample_paths_vecchia).  The walk assembles every node's inputs and
lets likelihood nodes sample; drawing a GP node (statistics, drawer, generator) is the caller's `draw`."""
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
    """The input of first-layer node nd at the rows xd (M, Dx) of the hierarchy's input: its input_dim, then its connect columns."""
    xin = cols(xd, nd.input_dim)
    return xin if nd.connect is None else torch.cat((xin, cols(xd, nd.connect)), 1)


def per_path(t, P):
    """(M, D) shared by every path as (P, M, D); a (P, M, D) tensor as it is."""
    return t if t.dim() == 3 else t[None].expand(P, *t.shape)


def walk(e, structs, J, m, z, first, draw):
    """Paths of a DGP hierarchy, layer by layer: yields each layer's (P, M, K) device tensor, P = len(structs) * J, the
    last one the hierarchy's output (a Categorical top: its class probabilities).  structs[s] is the structure behind paths
    s*J .. (s+1)*J - 1 (an emulator: its all_layer for every imputation; an lgp: system s's snapshot); m the hierarchy's
    input, (M, D) shared by every path or (P, M, D); z its external input (M, Dz) or None; first(nd) the input of
    first-layer node nd, (M, D') or (P, M, D').  A deeper node sees its input_dim columns of the layer below plus its
    `connect` columns: of m when every path shares it, else split over m and z as lgp.dgp_pred does.
    draw(il, j, nodes, xin) -> (P, M) draws GP node j of layer il (nodes[s] = structs[s][il][j]) at xin; likelihood nodes
    sample from the path's latents after the GP nodes of their layer (structs[p // J]'s node for path p)."""
    S, L = len(structs), len(structs[0])
    P, M = S * J, m.shape[-2]
    internal, external = structs[0][0][0].input_dim, structs[0][0][0].connect
    prev = None
    for il, layer in enumerate(structs[0]):
        if il == L - 1 and len(layer) == 1 and getattr(layer[0], 'name', None) == 'Categorical':
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
                parts = [cols(prev, nd.input_dim)]
                if nd.connect is not None and m.dim() == 2:
                    parts.append(per_path(cols(m, nd.connect), P))
                elif nd.connect is not None:
                    i1, i2 = connect_split(nd.connect, il == L - 1, m.shape[-1], internal, external)
                    if i1.size:
                        parts.append(cols(m, i1))
                    if i2.size:
                        parts.append(per_path(cols(z, i2), P))
                xin = torch.cat(parts, 2)
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
