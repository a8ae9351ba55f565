"""Typed Python front of the C-ABI (include/dgp_amd.h).

`Engine` owns one libdgp_amd context bound to a device and a HIP stream.  Device
memory is plain torch tensors (torch is plumbing here: allocation, streams,
torch.distributed); every numerical operation is a HIP kernel behind the C-ABI.
Host-side small parameters (lengthscales, angles) are numpy arrays.
"""
import ctypes as C

import numpy as np
import torch

import os

from . import _lib
from ._lib import lib, KIND

_NO_PINNED_UPLOAD = os.environ.get('DGPAMD_PINNED_UPLOAD') == '0'   # (comparison runs: pageable, blocking uploads)
_POISON_ALL = os.environ.get('DGPAMD_POISON_LDS') == '2'
_POISON_HBM = os.environ.get('DGPAMD_POISON_HBM') == '1'   # (debugging: fresh device buffers are filled with 0xFF bytes -- NaNs as doubles)   # (debugging: NaNs into every CU's LDS before every library call)


class DgpAmdError(RuntimeError):
    pass


class HandoffError(DgpAmdError):
    """The one-launch factorisation gave up waiting for another workgroup (its workgroups were not co-resident: a device
    shared with another process, a debugger, a time-sliced partition).  Not a numerical failure; the per-block-step
    factorisation (Engine.set_potrf_mode(0)) has no such waits -- dgp.train retries the iteration once through it."""


def raise_not_pd(info):
    """A non-zero factorisation status as the exception it stands for.  info > 0: LAPACK's index of the first
    non-positive pivot -> numpy.linalg.LinAlgError, the reference's signal (dgp.train restarts on it, compute_stats
    falls back to pinvh).  info < 0: a bounded in-kernel spin gave up (a lost workgroup hand-off) -- a device problem,
    never a numerical one, so it must not be swallowed by those recovery paths: DgpAmdError."""
    info = int(info)
    if info < 0:
        raise HandoffError('factorisation: an in-kernel hand-off timed out (info = %d); this is not a numerical failure' % info)
    raise np.linalg.LinAlgError('%d-th leading minor of the array is not positive definite' % info)


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))


def _f64_shapes(message, *pairs):
    """ValueError(message) unless every (tensor, shape) of pairs is a contiguous float64 tensor of that shape (None: any size)."""
    for t, shape in pairs:
        if len(t.shape) != len(shape) or any(n is not None and n != m for n, m in zip(shape, t.shape)) or \
                t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(message)


class Engine:
    def __init__(self, device=0, stream=None):
        if not torch.cuda.is_available():
            raise DgpAmdError('dgp_amd needs a HIP device: torch.cuda.is_available() is False and there is no CPU path')
        self.device = torch.device('cuda', device)
        torch.cuda.set_device(self.device)
        if stream is None:
            # Use the thread's CURRENT torch stream so that torch's copies / allocator and the library's launches
            # are ordered on one stream (every engine created in a thread without an explicit stream shares it).
            # hipGraph capture is illegal on the null stream: if that is the current one, switch the thread to a
            # side stream first.
            stream = torch.cuda.current_stream(self.device)
            if stream.cuda_stream == 0:
                stream = torch.cuda.Stream(self.device)
                torch.cuda.set_stream(stream)
        self._torch_stream = stream
        h = C.c_void_p()
        rc = lib.dgpamd_create(int(device), C.c_void_p(self._torch_stream.cuda_stream), C.byref(h))
        if rc != 0:
            raise DgpAmdError('dgpamd_create failed (rc=%d)' % rc)
        self.h = h
        self._ws = {}

    def close(self):
        if getattr(self, 'h', None):
            lib.dgpamd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ utils
    def _enter(self):
        """Called before every library call.  The library launches on THIS engine's stream; torch work the caller
        queued on another current stream (a different thread, a user's torch.cuda.stream block) is ordered before it by
        an event wait, and _chk() orders the caller's stream after the call again.  The creating thread's current
        stream IS the engine's stream, so both are no-ops there.  Returns None (used as `_enter() or lib.f(...)`)."""
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self._torch_stream.cuda_stream:
            self._torch_stream.wait_stream(cur)
            self._foreign = cur
        if _POISON_ALL:
            lib.dgpamd_debug_poison_lds(self.h)
        return None

    def _chk(self, rc):
        f = getattr(self, '_foreign', None)
        if f is not None:
            self._foreign = None
            f.wait_stream(self._torch_stream)
        if rc != 0:
            exc = self.__dict__.pop('_reduce_exc', None)
            if exc is not None:   # (an exception inside the reduce hook: the library call it interrupted has failed with it)
                raise exc
            raise DgpAmdError('libdgp_amd rc=%d: %s' % (rc, lib.dgpamd_last_error(self.h).decode()))

    def sync(self):
        self._chk(lib.dgpamd_sync(self.h))

    def tuning(self, name):
        """The value of one DGPAMD_* switch of the C library as this engine's context found it when it was created (a context keeps the
        switches it was created under).  0 for an unset switch whose default depends on the call; an unknown name raises."""
        v = C.c_int64()
        self._chk(lib.dgpamd_tuning_get(self.h, name.encode(), C.byref(v)))
        return v.value

    def set_linkgp_direct(self, enable):
        """Matern linked-GP J factor: reference's direct expression (True) or its separable form (default)."""
        self._chk(self._enter() or lib.dgpamd_set_linkgp_direct(self.h, 1 if enable else 0))

    def set_graphs(self, enable):
        self._chk(self._enter() or lib.dgpamd_set_graphs(self.h, 1 if enable else 0))

    def set_potrf_mode(self, mode):
        """1 (default): the factorisation is one persistent dataflow launch; 0: one launch per 64-column block step."""
        self._chk(self._enter() or lib.dgpamd_set_potrf_mode(self.h, int(mode)))

    def stream(self):
        """Context manager making this engine's HIP stream torch's current stream (so that torch's
        allocator and copies are ordered with the library's launches)."""
        return torch.cuda.stream(self._torch_stream)

    def tensor(self, a, dtype=torch.float64):
        """numpy -> device.  Through page-locked memory of torch's caching host allocator and an asynchronous copy: the call
        returns when the bytes are staged, not when the stream has reached the copy (a pageable upload waits for every kernel
        queued before it -- 1 to 2.5 ms per call inside the Vecchia I-step's set-up at n = 50 000)."""
        a = np.asarray(a)
        if self.device.type != 'cuda' or a.size == 0 or _NO_PINNED_UPLOAD:
            a = np.ascontiguousarray(a)
            if not a.flags.writeable:
                a = a.copy()
            return torch.as_tensor(a, dtype=dtype).to(self.device, non_blocking=False)
        pin = torch.empty(a.shape, dtype=dtype, pin_memory=True)
        np.copyto(pin.numpy(), a, casting='unsafe')
        return pin.to(self.device, non_blocking=True)   # (the allocator keeps the block until the copy has run)

    def empty(self, *shape, dtype=torch.float64):
        t = torch.empty(*shape, dtype=dtype, device=self.device)
        if _POISON_HBM and t.numel():   # (debugging: whatever is read before it is written shows up as NaN / -1)
            t.view(torch.uint8).fill_(255)
        return t

    def zeros(self, *shape, dtype=torch.float64):
        return torch.zeros(*shape, dtype=dtype, device=self.device)

    def workspace(self, key, nbytes):
        """Cached byte workspace (grown on demand) -- no allocation inside hot loops."""
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            t = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            if _POISON_HBM:
                t.fill_(255)
            self._ws[key] = t
        return t

    @staticmethod
    def padded_dim(n):
        return int(lib.dgpamd_padded_dim(int(n)))

    def event(self):
        e = C.c_void_p()
        self._chk(self._enter() or lib.dgpamd_event_create(self.h, C.byref(e)))
        return e

    def record(self, ev):
        self._chk(self._enter() or lib.dgpamd_event_record(self.h, ev))

    def elapsed_ms(self, start, stop):
        ms = C.c_float()
        self._chk(self._enter() or lib.dgpamd_event_elapsed_ms(self.h, start, stop, C.byref(ms)))
        return float(ms.value)

    PROF = dict(kmatrix=1, potrf_diag=2, trsm=3, syrk=4, trtri=5, lauum=6, grad=7, linkgp_j=8, gp_quad=9)

    def prof_enable(self, name):
        self._chk(self._enter() or lib.dgpamd_prof_enable(self.h, self.PROF[name] if name else 0))

    def prof_event_overhead_us(self):
        v = C.c_double()
        self._chk(self._enter() or lib.dgpamd_prof_event_overhead_us(self.h, C.byref(v)))
        return float(v.value)

    def prof_collect(self):
        """(launches, total_ms, algorithmic work) of the launches timed since prof_enable."""
        n, ms, w = C.c_int64(), C.c_double(), C.c_double()
        self._chk(self._enter() or lib.dgpamd_prof_collect(self.h, C.byref(n), C.byref(ms), C.byref(w)))
        return int(n.value), float(ms.value), float(w.value)

    # --------------------------------------------------------------- kernels
    @staticmethod
    def _colmap(colmap, Dl):
        if colmap is None:
            return None, None
        cm = np.ascontiguousarray(np.asarray(colmap, dtype=np.int32))
        assert cm.shape == (Dl,)
        return cm, _hp(cm)

    def kmatrix(self, kind, Xloc, colmap, Xglob, length, nugget, W=None, out=None, full=True, Y=None, batch=1):
        """K (full=True: n x n, both triangles; full=False: augmented Np x Np buffer with rows of Y).
        Xloc: (batch?, n, ldloc) tensor; colmap: gathered columns (None = all)."""
        n, ldloc = Xloc.shape[-2], Xloc.shape[-1]
        Dl = ldloc if colmap is None else len(colmap)
        Dg = 0 if Xglob is None else Xglob.shape[1]
        cm, cmp_ = self._colmap(colmap, Dl)
        length = _f64(length)
        stride_loc = n * ldloc if Xloc.dim() == 3 else 0
        if full:
            # (a caller's `out` may be a view of wider rows, e.g. buf[:, :n] of an (n, ld) buffer with 8 ld a multiple of 128 bytes:
            #  rows that start on 128-byte lines let every tile store whole lines -- 0.55 -> 0.72 of HBM for the stores alone at
            #  n = 5000, profiles/r05_kmatrix_store_shapes.txt)
            ld = n if out is None else int(out.stride(-2))
            r = 0
            if out is not None:   # (a transposed or narrow view would be written in a layout the caller does not expect)
                if out.stride(-1) != 1 or ld < n or out.shape[-1] < n or out.shape[-2] < n:
                    raise ValueError('kmatrix: `out` needs unit column stride and rows of at least n entries (strides %s, n = %d)' % (tuple(out.stride()), n))
                if batch > 1 and (out.dim() != 3 or out.stride(0) < n * ld):
                    raise ValueError('kmatrix: a batched `out` is (batch, n, ld) with matrices that do not overlap')
        else:
            ld = self.padded_dim(n)
            r = 0 if Y is None else (1 if Y.dim() == 1 else Y.shape[-2])
        if out is None:
            out = self.empty((batch, ld, ld) if batch > 1 else (ld, ld))
        stride_k = (ld * ld if (out.dim() < 3 or not full) else int(out.stride(0))) if batch > 1 else 0
        stride_y = 0
        if Y is not None and Y.dim() == 3:
            stride_y = Y.shape[-2] * Y.shape[-1]
        self._chk(self._enter() or lib.dgpamd_kmatrix(self.h, KIND[kind], n, _dp(Xloc), ldloc, stride_loc, cmp_, Dl, _dp(Xglob), Dg,
                                     _hp(length), len(length), float(nugget), _dp(W), _dp(out), ld, stride_k,
                                     1 if full else 0, _dp(Y), n, stride_y, r, batch))
        return out

    def potrf_workspace(self, n, batch):
        return self.workspace(('potrf', n, batch), lib.dgpamd_potrf_workspace(n, batch))

    def potrf(self, n, A, batch=1, work=None):
        """In-place factorisation of augmented buffers.  Returns (logdet, info) device tensors."""
        Np = self.padded_dim(n)
        if work is None:
            work = self.potrf_workspace(n, batch)
        logdet = self.empty(batch)
        info = self.empty(batch, dtype=torch.int32)
        self._chk(self._enter() or lib.dgpamd_potrf(self.h, n, _dp(A), Np * Np, batch, _dp(logdet), _dp(info), _dp(work)))
        return logdet, info

    def potrf_inv(self, n, A, T, S, batch=1, work=None):
        """Factorisation and inverse in one sweep (dgpamd_potrf_inv): A -> L, T -> L^-T, S -> K^-1 (lower tiles,
        row n = -alpha^T).  Returns (logdet, info) device tensors."""
        Np = self.padded_dim(n)
        if work is None:
            work = self.potrf_workspace(n, batch)
        logdet = self.empty(batch)
        info = self.empty(batch, dtype=torch.int32)
        self._chk(self._enter() or lib.dgpamd_potrf_inv(self.h, n, _dp(A), _dp(T), _dp(S), Np * Np, batch, _dp(logdet), _dp(info), _dp(work)))
        return logdet, info

    def aug_quad(self, n, A, batch, r):
        Np = self.padded_dim(n)
        out = self.empty(batch, r, r)
        self._chk(self._enter() or lib.dgpamd_aug_quad(self.h, n, _dp(A), Np * Np, batch, r, _dp(out)))
        return out

    def loglik_finish(self, n, A, logdet, scale, batch=1):
        """ll (batch,) of buffers assembled with their y row and factored by another call (dgpamd_loglik_finish)."""
        Np = self.padded_dim(n)
        ll = self.empty(batch)
        self._chk(self._enter() or lib.dgpamd_loglik_finish(self.h, n, _dp(A), Np * Np, batch, _dp(logdet), float(scale), _dp(ll)))
        return ll

    def loglik(self, kind, Xloc, colmap, Xglob, length, nugget, scale, y, W=None, batch=1, A=None, ll=None, info=None):
        """Batched ESS target (kernel_class.py:481-492).  Returns (ll, info) device tensors (no sync)."""
        n, ldloc = Xloc.shape[-2], Xloc.shape[-1]
        Dl = ldloc if colmap is None else len(colmap)
        Dg = 0 if Xglob is None else Xglob.shape[1]
        cm, cmp_ = self._colmap(colmap, Dl)
        length = _f64(length)
        Np = self.padded_dim(n)
        if A is None:
            A = self.workspace(('loglikA', n, batch), batch * Np * Np * 8)
        work = self.potrf_workspace(n, batch)
        if ll is None:
            ll = self.empty(batch)
        if info is None:
            info = self.empty(batch, dtype=torch.int32)
        stride_loc = n * ldloc if Xloc.dim() == 3 else 0
        self._chk(self._enter() or lib.dgpamd_loglik(self.h, KIND[kind], n, _dp(Xloc), ldloc, stride_loc, cmp_, Dl, _dp(Xglob), Dg,
                                    _hp(length), len(length), float(nugget), _dp(W), float(scale), _dp(y), _dp(A),
                                    Np * Np, batch, _dp(ll), _dp(info), _dp(work)))
        return ll, info

    def trmv_lower(self, n, L, scale, z, batch=1, out=None, shared=False):
        """out[b] = sqrt(scale[b]) L_b z[b]; shared: one factored buffer L for the whole batch (batch stride 0)."""
        Np = self.padded_dim(n)
        sc = _f64(scale)
        if len(sc) == 1 and batch > 1:
            sc = np.repeat(sc, batch)
        if out is None:
            out = self.empty(batch, n)
        self._chk(self._enter() or lib.dgpamd_trmv_lower(self.h, n, _dp(L), 0 if shared else Np * Np, _hp(sc), _dp(z), _dp(out),
                                                          batch))
        return out

    def ess_propose(self, F, NU, thetas, out=None):
        n, M = F.shape
        th = _f64(thetas)
        B = len(th)
        if out is None:
            out = self.empty(B, n, M)
        self._chk(self._enter() or lib.dgpamd_ess_propose(self.h, n, M, _dp(F), _dp(NU), _hp(th), B, _dp(out)))
        return out

    def potri(self, n, A, Ainv, r, work, batch=1):
        Np = self.padded_dim(n)
        self._chk(self._enter() or lib.dgpamd_potri_batched(self.h, n, _dp(A), _dp(Ainv), Np * Np if batch > 1 else 0, r, batch, _dp(work)))
        return Ainv

    def grad_reduce(self, kind, Xloc, colmap, Xglob, length, nugget, nugget_est, Ainv, W=None):
        n, ldloc = Xloc.shape[-2], Xloc.shape[-1]
        Dl = ldloc if colmap is None else len(colmap)
        Dg = 0 if Xglob is None else Xglob.shape[1]
        cm, cmp_ = self._colmap(colmap, Dl)
        length = _f64(length)
        P = (1 if len(length) == 1 else Dl + Dg) + (1 if nugget_est else 0)
        work = self.workspace(('grad', n, P), lib.dgpamd_grad_workspace(n, P))
        out = self.empty(2 * P)
        self._chk(self._enter() or lib.dgpamd_grad_reduce(self.h, KIND[kind], n, _dp(Xloc), ldloc, cmp_, Dl, _dp(Xglob), Dg, _hp(length),
                                         len(length), float(nugget), _dp(W), 1 if nugget_est else 0, _dp(Ainv), _dp(out),
                                         _dp(work)))
        return out, P

    def gemv(self, A, x, out=None):
        rows, cols = A.shape
        if out is None:
            out = self.empty(rows)
        self._chk(self._enter() or lib.dgpamd_gemv(self.h, rows, cols, _dp(A), A.stride(0), _dp(x), _dp(out)))
        return out

    def pinvh(self, K):
        """Pseudo-inverse of the symmetric matrix K (n x n device tensor) with scipy.linalg.pinvh's rule: eigenvalues
        of magnitude <= n eps max|eigenvalue| are dropped.  The rare fallback of `compute_stats` when R is not
        numerically positive definite (kernel_class.py:745-751); the eigen-decomposition is the vendor solver's
        (hipSOLVER through torch.linalg.eigh) and runs on the device like everything else."""
        s, u = torch.linalg.eigh(K)
        cut = s.abs().max() * K.shape[0] * torch.finfo(K.dtype).eps
        inv = torch.where(s.abs() > cut, 1.0 / s, torch.zeros_like(s))
        return (u * inv) @ u.T

    def post_het(self, K, scale, gamma_eff, y_eff, sd):
        """One draw of the mean latent of a heteroskedastic Gaussian likelihood from its exact conditional posterior
        (Hetero.post_het1 / post_het2, likelihood_class.py:184-243) with v = scale K:
            f = K alpha + u,   (K + diag(gamma_eff / scale)) alpha = y_eff - u - w,
            u = chol(v) sd[:, 0],   w = sqrt(gamma_eff) sd[:, 1].
        K: (n, n) full kernel matrix (device); gamma_eff, y_eff: (n,) device; sd: (n, 2) device.  Two factorisations:
        one for u, one (with the right-hand side riding along, inverse in the same sweep) for alpha."""
        n = K.shape[0]
        Np = self.padded_dim(n)
        A = self.workspace(('hetA', n), Np * Np * 8).view(torch.float64).view(Np, Np)
        T = self.workspace(('hetT', n), Np * Np * 8).view(torch.float64).view(Np, Np)
        S = self.workspace(('hetS', n), Np * Np * 8).view(torch.float64).view(Np, Np)
        work = self.potrf_workspace(n, 1)
        A.zero_()
        A[:n, :n] = K
        _, info1 = self.potrf(n, A, work=work)
        u = self.trmv_lower(n, A, [float(scale)], sd[:, 0].contiguous())[0]
        w = torch.sqrt(gamma_eff) * sd[:, 1]
        A.zero_()
        A[:n, :n] = K
        A.diagonal()[:n] += gamma_eff / float(scale)
        A[n, :n] = y_eff - u - w
        _, info2 = self.potrf_inv(n, A, T, S, work=work)
        alpha = -S[n, :n]
        f = self.gemv(K, alpha.contiguous()) + u
        bad = int(self.fetch(info1)[0]) or int(self.fetch(info2)[0])
        if bad:
            raise_not_pd(bad)
        return f

    def fetch(self, t):
        """Device tensor -> numpy array through the library's pinned staging buffer (one stream sync; cheaper than
        torch's .cpu() for the few bytes a sampler / optimiser step returns)."""
        t = t.contiguous()
        out = np.empty(tuple(t.shape), dtype={torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64}[t.dtype])
        self._chk(self._enter() or lib.dgpamd_fetch(self.h, _dp(t), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    MAILBOXES = 8
    # who uses which mailbox (the ranges must not overlap: a slot that still holds a result refuses the next post):
    MSTEP_SLOTS = 2      # 0 .. MSTEP_SLOTS-1: the lock-step M-step's optimiser groups in flight (mstep.py); kernel.ord_nn's default is 0,
                         # outside an M-step
    DETACH_SLOT0 = 2     # DETACH_SLOT0 + l: the imputer's deferred detach posts hidden layer l's latents (imputation.py)
    assert MSTEP_SLOTS <= DETACH_SLOT0 < MAILBOXES

    def use_dist_reduce(self):
        """Install dgp_amd.dist's all-reduce as the context's reduce hook (dgpamd_set_reduce_hook): the queued I-step of a model
        whose Vecchia likelihood rows are split over ranks sums every batch's partial sums over the ranks on the stream,
        between the row launch and the accept / shrink decision.  Idempotent."""
        if getattr(self, '_reduce_cb', None) is not None:
            return
        from . import dist as ddist
        HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)

        def hook(user, ptr, count):
            try:
                t = self._view_of(int(ptr), int(count))
                with torch.cuda.stream(self._torch_stream):
                    ddist.allreduce_sum(t)
                return 0
            except BaseException as exc:   # noqa: BLE001  (never unwind through the C frames: the call fails, _chk re-raises)
                self._reduce_exc = exc
                return 1
        self._reduce_cb = HOOK(hook)   # (kept alive with the engine)
        self._chk(self._enter() or lib.dgpamd_set_reduce_hook(self.h, C.cast(self._reduce_cb, C.c_void_p), None))

    def _view_of(self, ptr, count):
        """float64 view of `count` doubles at device address `ptr` inside one of the engine's workspaces."""
        for t in self._ws.values():
            base = t.data_ptr()
            if base <= ptr and ptr + 8 * count <= base + t.numel() * t.element_size():
                off = ptr - base
                return t.view(torch.uint8)[off:off + 8 * count].view(torch.float64)
        raise DgpAmdError('reduce hook: the buffer is not inside a workspace of this engine')

    def post(self, t, slot):
        """First half of fetch(): queue the copy of device tensor t into mailbox `slot` (0..7) behind everything queued so
        far and return a token at once (dgpamd_post).  Launches made afterwards do not delay it."""
        t = t.contiguous()
        self._chk(self._enter() or lib.dgpamd_post(self.h, _dp(t), t.numel() * t.element_size(), int(slot)))
        return (int(slot), tuple(t.shape), t.dtype, t)   # (t is kept alive until collect())

    def collect(self, token):
        """Second half: wait for THAT copy (not for the stream) and return the numpy array (dgpamd_collect)."""
        slot, shape, dtype, _ = token
        out = np.empty(shape, dtype={torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64}[dtype])
        self._chk(self._enter() or lib.dgpamd_collect(self.h, slot, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def discard(self, token):
        """Wait for a posted copy and drop it (the mailbox is free again)."""
        self._chk(self._enter() or lib.dgpamd_collect(self.h, token[0], None, 0))

    def fetch_ll_info(self, ll, info):
        """(ll float64 (B,), info int32 (B,)) device tensors -> two numpy arrays with ONE synchronisation."""
        B = ll.numel()
        buf = np.empty(12 * B, dtype=np.uint8)
        self._chk(self._enter() or lib.dgpamd_fetch2(self.h, _dp(ll), 8 * B, _dp(info), 4 * B, buf.ctypes.data_as(C.c_void_p)))
        return buf[:8 * B].view(np.float64), buf[8 * B:].view(np.int32)

    def linkgp_cells(self, kind, W_host, Wg, Rinv, ry):
        """Prediction statistics of a linked Matern-2.5 node with the training points grouped by cells (cell_order): the
        pair kernel then needs one record product instead of two for about half of its work (linkgp_Jsep_kernel's order
        classes).  W_host: (n x Dw) numpy inputs; Wg (n x Dz device or None), Rinv (ld x ld device, valid [:n, :n]), ry (n
        device) in the same row order.  Returns dict(W, Wg, Rinv, ry, pos) -- pos[i] = row of training point i in the new
        order (int32, what a leave-one-out call passes as `drop`) -- or None for kernels whose pair phase has no classes.
        The predictions are the same sums over all pairs (functions.py:421-494) in another order."""
        if kind != 'matern2.5' or os.environ.get('DGPAMD_LINK_CELLS', '1') == '0':
            return None
        n = len(W_host)
        p = cell_order(W_host)
        pd = torch.as_tensor(p, device=Rinv.device)
        pos = np.empty(n, dtype=np.int32)
        pos[p] = np.arange(n, dtype=np.int32)
        Rp = torch.zeros_like(Rinv)
        Rp[:n, :n] = Rinv[:n, :n][pd][:, pd]
        return dict(W=self.tensor(np.ascontiguousarray(np.asarray(W_host, dtype=float)[p])), Wg=None if Wg is None else Wg[pd].contiguous(),
                    Rinv=Rp, ry=ry[pd].contiguous(), pos=torch.as_tensor(pos, device=Rinv.device))

    def lik_loglik(self, lik, colmap, FP):
        """A likelihood node's log-likelihood of every candidate block FP[b] (B x n x M) -> device tensor (B,)
        (dgpamd_lik_loglik; imputation.py:71-78,91-106 -> <likelihood>.llik()).  lik: dict(kind, y, rep, classes, par) with
        device tensors y (observations) and rep (int64 latent row per observation, or None)."""
        B, n, M = FP.shape
        nd = _lib.Node()
        keep = _fill_lik_node(nd, colmap, lik, M)
        work = self.workspace(('likW', B), int(lib.dgpamd_lik_workspace(B)))
        out = self.empty(B)
        self._chk(self._enter() or lib.dgpamd_lik_loglik(self.h, C.byref(nd), n, M, _dp(FP), n * M, B, _dp(work), _dp(out)))
        del keep
        return out

    def ess_queue_plan(self, n, M, nodes, batch):
        return _EssQueue(self, n, M, nodes, batch)

    def ess_plan(self, n, M, kind, colmap, Xglob, length, nugget, W, y, batch):
        """Static arguments of dgpamd_ess_update for one upper GP node (see _EssPlan.run)."""
        return _EssPlan(self, n, M, kind, colmap, Xglob, length, nugget, W, y, batch)

    def llik_plan(self, n, specs):
        """Prepare the static part of dgpamd_llik_batch for a fixed set of GP nodes of size n.  specs: list of dicts
        kind, Xloc (n x ldloc tensor), Xglob (tensor or None), nlen, nugget_est, W (tensor or None), y (tensor).  Returns a
        plan whose per-call inputs are only the hyper-parameters (plan.set) -- no allocation, one C call per round."""
        return _LlikPlan(self, n, specs)

    def gp_predict(self, kind, x, Wtr, length, Rinv, ldr, ry, scale, nugget, mean=None, var=None):
        """ry: (n,) -> mean (M,) ; ry: (S, n) -> mean (S, M).  var is (M,) either way."""
        M, D = x.shape
        n = Wtr.shape[0]
        length = _f64(length)
        nry = 1 if ry.dim() == 1 else ry.shape[0]
        work = self.workspace(('gp', n, M), lib.dgpamd_gp_workspace(n, M))
        if mean is None:
            mean = self.empty(M) if ry.dim() == 1 else self.empty(nry, M)
        if var is None:
            var = self.empty(M)
        self._chk(self._enter() or lib.dgpamd_gp_predict(self.h, KIND[kind], n, M, D, _dp(x), _dp(Wtr), _hp(length), len(length), _dp(Rinv),
                                        ldr, _dp(ry), nry, float(scale), float(nugget), _dp(mean), _dp(var), _dp(work)))
        return mean, var

    def joint_cov(self, kind, x, W, Linv, y, length, scale, nugget, group=None, A=None, mean=None):
        """Joint posterior covariance and mean of test points (dgpamd_joint_cov).  x: (batch, M, D) or (M, D); W: (G, n, D)
        or (n, D); Linv: (G, ld, ld) or (ld, ld) with L^-1 in its lower tiles; y: (G, r, n), (r, n) or None; group: host
        ints (batch,) picking each item's W / Linv / y (None: all 0).  A W, Linv or y with one group (2-d, or a leading
        dimension of 1) is shared by all G groups (group stride 0).  Returns (A, mean): A (batch, Mp, Mp) dgpamd_potrf
        buffers holding scale (K** + nugget I - V^T V), Mp = padded_dim(M); mean (batch, M, r) or None."""
        xb = x if x.dim() == 3 else x[None]
        Wb = W if W.dim() == 3 else W[None]
        Lb = Linv if Linv.dim() == 3 else Linv[None]
        batch, M, D = xb.shape
        r = 0 if y is None else y.shape[-2]
        yb = None if y is None else (y if y.dim() == 3 else y[None])
        G, n = max(Wb.shape[0], Lb.shape[0], 1 if yb is None else yb.shape[0]), Wb.shape[1]
        assert Wb.shape[2] == D and Wb.shape[0] in (1, G) and Lb.shape[0] in (1, G)
        assert yb is None or (yb.shape[0] in (1, G) and yb.shape[2] == n)
        for t in (xb, Wb, Lb) + (() if yb is None else (yb,)):
            assert t.is_contiguous() and t.dtype == torch.float64
        length = _f64(length)
        Mp = self.padded_dim(M)
        g = np.zeros(batch, dtype=np.int32) if group is None else np.ascontiguousarray(np.asarray(group, dtype=np.int32))
        assert g.shape == (batch,)
        if A is None:
            A = self.empty(batch, Mp, Mp)
        if mean is None and r > 0:
            mean = self.empty(batch, M, r)
        work = self.workspace(('joint',), lib.dgpamd_joint_workspace(n, M, r, batch))
        ldl = Lb.shape[-1]
        sw, sl = (n * D if Wb.shape[0] > 1 else 0), (Lb.shape[-2] * ldl if Lb.shape[0] > 1 else 0)
        sy = r * n if yb is not None and yb.shape[0] > 1 else 0
        self._chk(self._enter() or lib.dgpamd_joint_cov(self.h, KIND[kind], n, M, D, r, batch, _dp(xb), M * D, _hp(g), G, _dp(Wb),
                                                         sw, _dp(Lb), ldl, sl, _dp(yb), sy, _hp(length),
                                                         len(length), float(scale), float(nugget), _dp(A), Mp * Mp, _dp(mean),
                                                         _dp(work)))
        return A, mean

    def mvn_paths(self, L, mean, E, rep=1, out=None):
        """out_b = mean_b(:, q // rep) + L_b E_b (dgpamd_mvn_paths).  L: (batch, Mp, Mp) factored joint_cov buffers;
        E: (batch, M, c) standard normals; mean: (batch, M, c // rep) or None.  Returns out (batch, M, c)."""
        batch, M, c = E.shape
        Mp = self.padded_dim(M)
        assert L.shape[-1] == Mp and L.is_contiguous() and E.is_contiguous()
        assert mean is None or (mean.is_contiguous() and mean.shape == (batch, M, c // rep))
        if out is None:
            out = self.empty(batch, M, c)
        sm = 0 if mean is None else M * (c // rep)
        self._chk(self._enter() or lib.dgpamd_mvn_paths(self.h, M, c, rep, batch, _dp(L), Mp * Mp, _dp(mean), sm, _dp(E), M * c,
                                                         _dp(out), M * c))
        return out

    def _pathfun_call(self, fn, kind, x, W, Omega, b, theta, v, length, scale, group, outs):
        """The checks and the argument list that dgpamd_pathfun_eval and dgpamd_pathfun_grad share; outs: the output tensors."""
        P, F = theta.shape
        M, D = x.shape[-2:]
        Wb = None if W is None else (W if W.dim() == 3 else W[None])
        n = 0 if Wb is None else Wb.shape[1]
        G = 1 if Wb is None else Wb.shape[0]
        assert x.dim() == 2 or x.shape[0] == P
        assert Omega.shape == (F, D) and b.shape == (F,) and (n == 0 or (v is not None and v.shape == (P, n) and Wb.shape[2] == D))
        for t in (x, Wb, Omega, b, theta, v if n else None):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float64)
        length = _f64(length)
        g = None if group is None else np.ascontiguousarray(np.asarray(group, dtype=np.int32))
        assert g is None or g.shape == (P,)
        outs = [self.empty(*shape) if o is None else o for o, shape in zip(outs, ((P, M), (P, M, D)))]
        for o, shape in zip(outs, ((P, M), (P, M, D))):
            assert o.shape == shape and o.is_contiguous()
        self._chk(self._enter() or fn(self.h, KIND[kind], n, M, D, F, P, _dp(x), M * D if x.dim() == 3 else 0,
                                      None if g is None else _hp(g), G, _dp(Wb), n * D, _dp(Omega), _dp(b), _dp(theta),
                                      _dp(v) if n else None, _hp(length), len(length), float(scale), *[_dp(o) for o in outs]))
        return outs

    def pathfun_eval(self, kind, x, W, Omega, b, theta, v, length, scale, group=None, out=None):
        """P function-valued draws of one GP node at M rows (dgpamd_pathfun_eval):
            out[p, m] = sqrt(scale) (sqrt(2/F) sum_f theta[p, f] cos(Omega[f] . x[m] + b[f]) + sum_i v[p, i] c(x[m], W_g(p)[i])).
        x: (M, D) shared by every path, or (P, M, D); W: (n, D), (G, n, D) or None (n = 0: the prior part alone); Omega
        (F, D), b (F,), theta (P, F), v (P, n) or None; group: host ints (P,) picking each path's W (None: all 0; shared x
        needs one group).  Returns out (P, M)."""
        return self._pathfun_call(lib.dgpamd_pathfun_eval, kind, x, W, Omega, b, theta, v, length, scale, group, [out])[0]

    def pathfun_grad(self, kind, x, W, Omega, b, theta, v, length, scale, group=None, out=None, grad=None):
        """pathfun_eval's draws and their input gradients in one pass (dgpamd_pathfun_grad): the arguments of pathfun_eval;
        returns (out (P, M), grad (P, M, D)), out bit for bit pathfun_eval's and grad[p, m, d] = d out[p, m] / d x[m, d]
        (x[p, m, d] for per-path x), in the node's own D input columns."""
        return tuple(self._pathfun_call(lib.dgpamd_pathfun_grad, kind, x, W, Omega, b, theta, v, length, scale, group, [out, grad]))

    def linkgp_predict(self, kind, m, v, z, Wtr, Wg, length, Rinv, ldr, ry, scale, nugget, mean=None, var=None,
                       drop=None):
        """drop (M,) int32 device tensor: leave training point drop[t] out of test point t's conditioning set."""
        M, Dw = m.shape
        Dz = 0 if z is None else z.shape[1]
        n = Wtr.shape[0]
        length = _f64(length)
        work = self.workspace(('link', n, M, Dw), lib.dgpamd_linkgp_workspace(n, M, Dw))
        if mean is None:
            mean = self.empty(M)
        if var is None:
            var = self.empty(M)
        if drop is not None:
            assert drop.dtype == torch.int32 and drop.numel() == M and drop.is_contiguous()
            self._chk(self._enter() or lib.dgpamd_linkgp_loo(self.h, KIND[kind], n, M, Dw, Dz, _dp(m), _dp(v), _dp(z), _dp(Wtr), _dp(Wg),
                                            _hp(length), len(length), _dp(Rinv), ldr, _dp(ry), _dp(drop), float(scale),
                                            float(nugget), _dp(mean), _dp(var), _dp(work)))
            return mean, var
        self._chk(self._enter() or lib.dgpamd_linkgp_predict(self.h, KIND[kind], n, M, Dw, Dz, _dp(m), _dp(v), _dp(z), _dp(Wtr), _dp(Wg),
                                            _hp(length), len(length), _dp(Rinv), ldr, _dp(ry), float(scale),
                                            float(nugget), _dp(mean), _dp(var), _dp(work)))
        return mean, var

    def moments_accumulate(self, mu, var, sum_mu, sum_m2):
        self._chk(self._enter() or lib.dgpamd_moments_accumulate(self.h, mu.numel(), _dp(mu), _dp(var), _dp(sum_mu), _dp(sum_m2)))

    def moments_finalize(self, S, sum_mu, sum_m2):
        self._chk(self._enter() or lib.dgpamd_moments_finalize(self.h, sum_mu.numel(), float(S), _dp(sum_mu), _dp(sum_m2)))

    # --------------------------------------------------------------- predictive mixture (csrc/mixture.hip)
    MIX_WHAT = dict(cdf=0, sf=1, logpdf=2)
    MIX_PATH = {None: 0, 'lds': 1, 'global': 2}
    MIX_MAXT = 32

    @staticmethod
    def _mix_components(mu, var):
        if mu.dim() != 2 or mu.shape != var.shape or mu.dtype != torch.float64 or var.dtype != torch.float64:
            raise ValueError('mixture: mu and var must be float64 tensors of one shape (S, count)')
        if mu.shape[0] < 1:
            raise ValueError('mixture: at least one component is needed')
        return mu.contiguous(), var.contiguous(), mu.shape[0], mu.shape[1]

    def mixture_eval(self, what, mu, var, y):
        """cdf / sf / logpdf (what: a key of Engine.MIX_WHAT) of the equal-weight mixtures of the S Gaussians N(mu[s, e], var[s, e]),
        e < count, at y: (count, T) one row of thresholds per entry, or (T,) thresholds shared by all entries.  Returns (count, T)."""
        mu, var, S, count = self._mix_components(mu, var)
        if y.dtype != torch.float64 or not (y.dim() == 1 or (y.dim() == 2 and y.shape[0] == count)) or y.shape[-1] < 1:
            raise ValueError('mixture: y must be a float64 tensor (count, T) or (T,), T >= 1')
        y = y.contiguous()
        T = y.shape[-1]
        out = self.empty(count, T)
        self._chk(self._enter() or lib.dgpamd_mixture_eval(self.h, self.MIX_WHAT[what], S, count, T, _dp(mu), _dp(var), _dp(y),
                                                          T if y.dim() == 2 else 0, _dp(out)))
        return out

    def mixture_quantile(self, mu, var, p, path=None):
        """out[e, t] = inf{q : F_e(q) >= p[t]} of the same mixtures; p: 1-d host array of probabilities in (0, 1).  Returns
        ((count, T) tensor, the number of results that reached the kernel's iteration limit -- expected 0).  path: None (the
        size of S decides), 'lds' or 'global' -- which of the two kernels runs (the same arithmetic)."""
        from scipy.special import ndtri
        mu, var, S, count = self._mix_components(mu, var)
        p = _f64(p)
        if p.size < 1 or not np.all((p > 0.0) & (p < 1.0)):
            raise ValueError('mixture: the probabilities must lie in (0, 1)')
        zp = np.ascontiguousarray(ndtri(p))
        out, info = self.empty(count, p.size), self.zeros(1, dtype=torch.int32)
        capped = 0
        for t0 in range(0, p.size, self.MIX_MAXT):
            T = min(self.MIX_MAXT, p.size - t0)
            part = out if T == p.size else self.empty(count, T)
            self._chk(self._enter() or lib.dgpamd_mixture_quantile(self.h, S, count, T, _dp(mu), _dp(var), _hp(p[t0:t0 + T]),
                                                                  _hp(zp[t0:t0 + T]), self.MIX_PATH[path], _dp(part), _dp(info)))
            if part is not out:
                out[:, t0:t0 + T] = part
            capped += int(self.fetch(info)[0]) if count else 0
        return out, capped

    def mixture_crps(self, mu, var, y, path=None):
        """CRPS of the same mixtures at the observations y (count,).  Returns (count,).  path as mixture_quantile's."""
        mu, var, S, count = self._mix_components(mu, var)
        if y.dtype != torch.float64 or y.dim() != 1 or y.shape[0] != count:
            raise ValueError('mixture: y must be a float64 tensor (count,)')
        y = y.contiguous()
        out = self.empty(count)
        self._chk(self._enter() or lib.dgpamd_mixture_crps(self.h, S, count, _dp(mu), _dp(var), _dp(y), self.MIX_PATH[path], _dp(out)))
        return out

    # --------------------------------------------------------------- pick-freeze sums (csrc/sobol.hip)
    def sobol_tiles(self, fA, fB, fAB, shift):
        """The per-tile pick-freeze sums of dgpamd_sobol_tiles.  fA, fB, fAB: (P, M, K) float64 device tensors, the paths at the
        rows of A, B and AB_i; shift (P, K).  fAB None: returns (ntiles, P, K, 4), the sums of g_A, g_B, g_A^2, g_B^2 over
        each tile of 64 rows, g = f - shift; else (ntiles, P, K, 2), the sums of g_B (g_AB - g_A) and (g_A - g_AB)^2."""
        if fA.dim() != 3:
            raise ValueError('sobol: the values must be (P, M, K)')
        P, M, K = fA.shape          # (an empty axis is the library's to refuse: DgpAmdError)
        for t, shape in ((fA, (P, M, K)), (fB, (P, M, K)), (fAB, (P, M, K)), (shift, (P, K))):
            if t is not None and (t.shape != shape or t.dtype != torch.float64 or not t.is_contiguous()):
                raise ValueError('sobol: fA, fB, fAB must be contiguous float64 tensors of one shape (P, M, K), shift (P, K)')
        partial = self.empty(-(-M // 64), P, K, 4 if fAB is None else 2)
        self._chk(self._enter() or lib.dgpamd_sobol_tiles(self.h, P, M, K, _dp(fA), _dp(fB), _dp(fAB), _dp(shift), _dp(partial)))
        return partial

    def sobol_add(self, partial, sums):
        """sums += the tiles of partial (ntiles, ...), one after the other in tile order (dgpamd_sobol_add); sums has the shape
        of one tile's entries and is updated in place."""
        if partial.shape[1:] != sums.shape:
            raise ValueError('sobol: sums must have the shape of one tile of partial')
        for t in (partial, sums):
            if t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError('sobol: partial and sums must be contiguous float64 tensors')
        self._chk(self._enter() or lib.dgpamd_sobol_add(self.h, partial.shape[0], sums.numel(), _dp(partial), _dp(sums)))
        return sums

    # --------------------------------------------------------------- gradient second moments (csrc/gradmom.hip)
    def gradmom_tiles(self, f, J, shift):
        """The per-tile sums of dgpamd_gradmom_tiles.  f (P, M, K), J (P, M, K, Dx), shift (P, K): contiguous float64 device
        tensors, the values and the Jacobian of the paths as the walk leaves them, 1 <= Dx <= 64.  Returns (ntiles, P, K, NC),
        NC = 2 + Dx + Dx (Dx + 1) / 2: over each tile of 64 rows the sums of g = f - shift and g^2, of J_d, and of J_d J_e for
        d <= e (the upper triangle packed row-major).  sobol_add adds the tiles onto running sums (P, K, NC)."""
        if f.dim() != 3 or J.dim() != 4:
            raise ValueError('gradmom: the values must be (P, M, K) and the Jacobian (P, M, K, Dx)')
        P, M, K = f.shape           # (an empty axis is the library's to refuse: DgpAmdError)
        Dx = J.shape[3]
        if not 1 <= Dx <= 64:
            raise ValueError('gradmom: the Jacobian must have 1 to 64 columns, got %d' % Dx)
        for t, shape in ((f, (P, M, K)), (J, (P, M, K, Dx)), (shift, (P, K))):
            if t.shape != shape or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError('gradmom: f (P, M, K), J (P, M, K, Dx) and shift (P, K) must be contiguous float64 tensors')
        partial = self.empty(-(-M // 64), P, K, 2 + Dx + Dx * (Dx + 1) // 2)
        self._chk(self._enter() or lib.dgpamd_gradmom_tiles(self.h, P, M, K, Dx, _dp(f), _dp(J), _dp(shift), _dp(partial)))
        return partial

    # --------------------------------------------------------------- box-constrained minimisation (csrc/boxmin.hip)
    BOXMIN = dict(running=0, gtol=1, ftol=2, maxiter=3, maxeval=4, linesearch=5, nan=6)

    @staticmethod
    def boxmin_workspace(Q, D, history):
        """Bytes of the state workspace of boxmin_step for Q problems of D columns (dgpamd_boxmin_workspace: a host-side
        formula); sizes that the step refuses raise ValueError."""
        nbytes = int(lib.dgpamd_boxmin_workspace(int(Q), int(D), int(history)))
        if nbytes == 0:
            raise ValueError('boxmin: need Q >= 1, 1 <= D <= %d and 1 <= history <= 16' % _lib.MAXD)
        return nbytes

    def boxmin_state(self, Q, D, history, lo, hi):
        """What one minimisation keeps between its boxmin_step calls: the opaque workspace, the box on the device and on the
        host, and the results x (Q, D), fun (Q,), status, n_iter, n_eval (Q,) int32 and running (1,) int32."""
        lo, hi = _f64(lo), _f64(hi)
        if lo.size != D or hi.size != D:
            raise ValueError('boxmin: lo and hi must hold D = %d bounds' % D)
        return dict(work=torch.empty(self.boxmin_workspace(Q, D, history), dtype=torch.uint8, device=self.device),
                    history=int(history), lo_h=lo, hi_h=hi, lo=self.tensor(lo), hi=self.tensor(hi),
                    x=self.empty(Q, D), fun=self.empty(Q), status=self.zeros(Q, dtype=torch.int32),
                    n_iter=self.zeros(Q, dtype=torch.int32), n_eval=self.zeros(Q, dtype=torch.int32),
                    running=self.zeros(1, dtype=torch.int32))

    def boxmin_step(self, state, f, J, x_trial, k=0, sign=1.0, maxiter=100, max_eval=420, gtol=1e-6, ftol=1e-12, first=False):
        """One transition of every problem's projected L-BFGS (dgpamd_boxmin_step).  state: boxmin_state's; f (Q, K) or
        (P, R, K) and J (Q, K, D) or (P, R, K, D): the walk's values and Jacobian at x_trial (Q, D) or (P, R, D), contiguous
        float64 device tensors, of which column k is read and multiplied by sign (+1 or -1); x_trial is overwritten with the
        next trial points.  first: initialise the state from x_trial.  The results are state's tensors, updated in place."""
        if x_trial.dim() not in (2, 3) or f.dim() != x_trial.dim() or J.dim() != x_trial.dim() + 1:
            raise ValueError('boxmin: x_trial must be (Q, D) or (P, R, D), f (..., K) and J (..., K, D) beside it')
        D, K = x_trial.shape[-1], f.shape[-1]
        lead = x_trial.shape[:-1]
        Q = int(np.prod(lead))
        _f64_shapes('boxmin: x_trial, f, J must be contiguous float64 tensors (..., D), (..., K), (..., K, D)',
                    (x_trial, (*lead, D)), (f, (*lead, K)), (J, (*lead, K, D)))
        sizes = dict(x=Q * D, fun=Q, status=Q, n_iter=Q, n_eval=Q, running=1, lo=D, hi=D)
        if state['work'].numel() < self.boxmin_workspace(Q, D, state['history']) or state['lo_h'].size != D or \
                state['hi_h'].size != D or any(state[name].numel() != count for name, count in sizes.items()):
            raise ValueError('boxmin: the state was made for another Q or D')
        self._chk(self._enter() or lib.dgpamd_boxmin_step(
            self.h, Q, D, K, int(k), float(sign), _dp(f), _dp(J), _dp(state['lo']), _dp(state['hi']), _hp(state['lo_h']),
            _hp(state['hi_h']), state['history'], int(maxiter), int(max_eval), float(gtol), float(ftol), 1 if first else 0,
            _dp(state['work']), _dp(x_trial), _dp(state['x']), _dp(state['fun']), _dp(state['status']), _dp(state['n_iter']),
            _dp(state['n_eval']), _dp(state['running'])))
        return x_trial

    # --------------------------------------------------------------- chains over a box (csrc/boxchain.hpp: boxmala.hip, boxhmc.hip)
    BOXMALA = dict(ok=0, nan=1)
    BOXHMC = BOXMALA

    @staticmethod
    def _chain_workspace(what, Q, D):
        nbytes = int(getattr(lib, 'dgpamd_%s_workspace' % what)(int(Q), int(D)))
        if nbytes == 0:
            raise ValueError('%s: need Q >= 1 and 1 <= D <= %d' % (what, _lib.MAXD))
        return nbytes

    def _chain_par(self, what, D, w, ybar, lo, hi, scale, prior_prec, prior_mean, n_slots=0):
        """(K, par_h) of the chains and of boxsmc's move: w (K), ybar (K), prior_prec (D, None: 0), prior_mean, scale, lo, hi."""
        w, ybar, lo, hi, scale = _f64(w), _f64(ybar), _f64(lo), _f64(hi), _f64(scale)
        pv = np.zeros(D) if prior_prec is None else _f64(prior_prec)
        pm = np.zeros(D) if prior_mean is None else _f64(prior_mean)
        K = w.size
        if K < 1 or ybar.size != K or any(a.size != D for a in (lo, hi, scale, pv, pm)) or n_slots < 0:
            raise ValueError('%s: w and ybar must hold K >= 1 entries; lo, hi, scale and the prior D = %d' % (what, D))
        return K, np.concatenate([w, ybar, pv, pm, scale, lo, hi])

    def _chain_state(self, what, Q, D, w, ybar, lo, hi, scale, prior_prec, prior_mean, n_slots):
        K, par = self._chain_par(what, D, w, ybar, lo, hi, scale, prior_prec, prior_mean, n_slots)
        return dict(work=torch.empty(self._chain_workspace(what, Q, D), dtype=torch.uint8, device=self.device), K=K,
                    n_slots=int(n_slots), par_h=par, par=self.tensor(par), h=self.empty(Q), logr=self.empty(Q),
                    status=self.zeros(Q, dtype=torch.int32), n_prop=self.zeros(Q, dtype=torch.int32),
                    n_acc=self.zeros(Q, dtype=torch.int32), xs=self.empty(max(int(n_slots), 1), D, Q),
                    lps=self.empty(max(int(n_slots), 1), Q))

    def _chain_step(self, what, state, f, J, x_trial, z, logu, h0, hmin, hmax, up, down, adapt, first, slot, last=None):
        """dgpamd_boxmala_step or dgpamd_boxhmc_step: the one call; last is the argument that the HMC step alone takes."""
        Q, D, K = self._chain_shapes(what, state, f, J, x_trial, z, logu)
        flags = (1 if adapt else 0, 1 if first else 0) + (() if last is None else (1 if last else 0,))
        self._chk(self._enter() or getattr(lib, 'dgpamd_%s_step' % what)(
            self.h, Q, D, K, _dp(f), _dp(J), _dp(state['par']), _hp(state['par_h']), _dp(z), _dp(logu), float(h0), float(hmin),
            float(hmax), float(up), float(down), *flags, int(slot), state['n_slots'], _dp(state['work']), _dp(x_trial),
            _dp(state['h']), _dp(state['logr']), _dp(state['xs']), _dp(state['lps']), _dp(state['status']), _dp(state['n_prop']),
            _dp(state['n_acc'])))
        return x_trial

    def _chain_shapes(self, what, state, f, J, x_trial, z, logu):
        """(Q, D, K) of a chain step's tensors after the checks that boxmala_step and boxhmc_step share."""
        if x_trial.dim() not in (2, 3) or f.dim() != x_trial.dim() or J.dim() != x_trial.dim() + 1:
            raise ValueError('%s: x_trial must be (Q, D) or (P, R, D), f (..., K) and J (..., K, D) beside it' % what)
        D, K = x_trial.shape[-1], f.shape[-1]
        lead = x_trial.shape[:-1]
        Q = int(np.prod(lead))
        _f64_shapes('%s: x_trial, f, J, z, logu must be contiguous float64 tensors (..., D), (..., K), (..., K, D), (..., D), (...)' % what,
                    (x_trial, (*lead, D)), (f, (*lead, K)), (J, (*lead, K, D)), (z, (*lead, D)), (logu, tuple(lead)))
        sizes = dict(h=Q, logr=Q, status=Q, n_prop=Q, n_acc=Q, xs=max(state['n_slots'], 1) * D * Q, lps=max(state['n_slots'], 1) * Q,
                     par=2 * K + 5 * D)
        if state['work'].numel() < self._chain_workspace(what, Q, D) or state['K'] != K or state['par_h'].size != 2 * K + 5 * D or \
                any(state[name].numel() != count for name, count in sizes.items()):
            raise ValueError('%s: the state was made for another Q, D or K' % what)
        return Q, D, K

    # MALA (csrc/boxmala.hip)
    @staticmethod
    def boxmala_workspace(Q, D):
        """Bytes of the state workspace of boxmala_step for Q chains of D columns (dgpamd_boxmala_workspace: a host-side
        formula); sizes that the step refuses raise ValueError."""
        return Engine._chain_workspace('boxmala', Q, D)

    def boxmala_state(self, Q, D, w, ybar, lo, hi, scale, prior_prec=None, prior_mean=None, n_slots=0):
        """What one run keeps between its boxmala_step calls: the opaque workspace; par, the target and the proposal on the
        device -- w (K), ybar (K), prior_prec (D, None: 0, the uniform prior), prior_mean (D), scale (D), lo (D), hi (D) -- and
        par_h, its host copy; h, logr (Q) and status, n_prop, n_acc (Q) int32; the samples xs (n_slots, D, Q) and lps
        (n_slots, Q), chain fastest."""
        return self._chain_state('boxmala', Q, D, w, ybar, lo, hi, scale, prior_prec, prior_mean, n_slots)

    def boxmala_step(self, state, f, J, x_trial, z, logu, h0=0.1, hmin=1e-10, hmax=1e2, up=1.0, down=1.0, adapt=False,
                     first=False, slot=-1):
        """One call of every chain's MALA state machine (dgpamd_boxmala_step).  state: boxmala_state's; f (Q, K) or (P, R, K)
        and J (Q, K, D) or (P, R, K, D): the walk's values and Jacobian at x_trial (Q, D) or (P, R, D); z (Q, D) or (P, R, D)
        and logu (Q,) or (P, R): this call's draws; all contiguous float64 device tensors.  x_trial is overwritten with the
        next trial points.  first: initialise the state from x_trial, the steps to h0.  adapt: multiply a chain's step by up
        after an acceptance and by down after a rejection, clamped to [hmin, hmax].  slot >= 0: store the sample."""
        return self._chain_step('boxmala', state, f, J, x_trial, z, logu, h0, hmin, hmax, up, down, adapt, first, slot)

    # HMC, reflecting walls (csrc/boxhmc.hip)
    @staticmethod
    def boxhmc_workspace(Q, D):
        """Bytes of the state workspace of boxhmc_step for Q chains of D columns (dgpamd_boxhmc_workspace: a host-side
        formula); sizes that the step refuses raise ValueError."""
        return Engine._chain_workspace('boxhmc', Q, D)

    def boxhmc_state(self, Q, D, w, ybar, lo, hi, scale, prior_prec=None, prior_mean=None, n_slots=0):
        """What one run keeps between its boxhmc_step calls: boxmala_state's fields with the workspace of the HMC step."""
        return self._chain_state('boxhmc', Q, D, w, ybar, lo, hi, scale, prior_prec, prior_mean, n_slots)

    def boxhmc_step(self, state, f, J, x_trial, z, logu, h0=0.1, hmin=1e-10, hmax=1e2, up=1.0, down=1.0, adapt=False,
                    first=False, last=False, slot=-1):
        """One call of every chain's HMC state machine (dgpamd_boxhmc_step): one leapfrog step of a trajectory, with the
        walls of the box reflecting.  The arguments are boxmala_step's.  first: initialise the state from x_trial, the steps
        to h0, and start a trajectory from the momenta z.  last: this call closes the trajectory -- the energy test against
        logu, the step's adaptation (adapt), then the start of the next trajectory from z.  Otherwise z and logu are not
        read.  slot >= 0: store the sample."""
        return self._chain_step('boxhmc', state, f, J, x_trial, z, logu, h0, hmin, hmax, up, down, adapt, first, slot, bool(last))

    # populations over a box (csrc/boxpop.hpp: boxsmc.hip, boxsus.hip)
    def _pop_sizes(self, what, made_for, state, x_trial, more, counts):
        """(P, R, D) of x_trial after the checks that boxsmc's and boxsus's calls share: x_trial's form, (P, R, D), then state
        against more(P, R, D), a check of the family's own, and counts(P, R, D, Q), a table name -> element count."""
        _f64_shapes('%s: x_trial must be a contiguous float64 tensor (P, R, D)' % what, (x_trial, (None, None, None)))
        P, R, D = x_trial.shape
        if state['P'] != P or state['R'] != R or not more(P, R, D) or \
                any(state[name].numel() != n or not state[name].is_contiguous() for name, n in counts(P, R, D, P * R).items()):
            raise ValueError('%s: the state was made for another %s' % (what, made_for))
        return P, R, D

    # tempered SMC (csrc/boxsmc.hip)
    BOXSMC = dict(ok=0, nan=1, max_stages=2)
    BOXSMC_MAXR = 8192

    @staticmethod
    def boxsmc_workspace(P, R, D):
        """Bytes of the workspace of boxsmc_move for P draws of R particles of D columns (dgpamd_boxsmc_workspace: a
        host-side formula); sizes that the calls refuse raise ValueError."""
        nbytes = int(lib.dgpamd_boxsmc_workspace(int(P), int(R), int(D)))
        if nbytes == 0:
            raise ValueError('boxsmc: need P >= 1, 1 <= R <= %d and 1 <= D <= %d' % (Engine.BOXSMC_MAXR, _lib.MAXD))
        return nbytes

    def boxsmc_state(self, P, R, D, w, ybar, lo, hi, scale, prior_prec=None, prior_mean=None, h0=0.1):
        """What one run keeps between its boxsmc_move and boxsmc_temper calls: the move's opaque workspace, par and par_h as
        boxmala_state; per particle x (D, Q) particle fastest, ll, lprior, h (filled with h0), logr (Q) and status, n_prop,
        n_acc (Q) int32, Q = P R; per draw beta (zeros), dbeta, log_evidence (zeros), stage_ess (P), draw_status (P) int32,
        anc (P, R) int32; running (1,) int32."""
        (K, par), Q = self._chain_par('boxsmc', D, w, ybar, lo, hi, scale, prior_prec, prior_mean), int(P) * int(R)
        return dict(work=torch.empty(self.boxsmc_workspace(P, R, D), dtype=torch.uint8, device=self.device), K=K, P=int(P),
                    R=int(R), par_h=par, par=self.tensor(par), x=self.zeros(D, Q), ll=self.zeros(Q), lprior=self.zeros(Q),
                    h=torch.full((Q,), float(h0), dtype=torch.float64, device=self.device), logr=self.zeros(Q),
                    status=self.zeros(Q, dtype=torch.int32), n_prop=self.zeros(Q, dtype=torch.int32),
                    n_acc=self.zeros(Q, dtype=torch.int32), beta=self.zeros(P), dbeta=self.zeros(P), log_evidence=self.zeros(P),
                    stage_ess=self.zeros(P), draw_status=self.zeros(P, dtype=torch.int32),
                    anc=self.zeros(P, R, dtype=torch.int32), running=self.zeros(1, dtype=torch.int32))

    def _boxsmc_sizes(self, state, x_trial):
        return self._pop_sizes(
            'boxsmc', 'P, R, D or K', state, x_trial,
            lambda P, R, D: state['work'].numel() >= self.boxsmc_workspace(P, R, D) and state['par_h'].size == 2 * state['K'] + 5 * D,
            lambda P, R, D, Q: dict(x=Q * D, ll=Q, lprior=Q, h=Q, logr=Q, status=Q, n_prop=Q, n_acc=Q, beta=P, dbeta=P, log_evidence=P,
                                    stage_ess=P, draw_status=P, anc=Q, running=1, par=2 * state['K'] + 5 * D))

    def boxsmc_move(self, state, f, J, x_trial, z, logu, hmin=1e-10, hmax=1e2, up=1.0, down=1.0, adapt=False, first=False,
                    last=False):
        """One call of every particle's tempered MALA state machine (dgpamd_boxsmc_move).  state: boxsmc_state's; f
        (P, R, K), J (P, R, K, D): the walk's values and Jacobian at x_trial (P, R, D); z (P, R, D), logu (P, R): this call's
        draws; all contiguous float64 device tensors.  first: a stage starts -- the state comes from x_trial under the
        draw's beta.  last: the stage ends -- x_trial <- x instead of a proposal.  adapt: as boxmala_step.  x_trial is
        overwritten with the next points to evaluate."""
        P, R, D = self._boxsmc_sizes(state, x_trial)
        K = state['K']
        _f64_shapes('boxsmc: f, J, z, logu must be contiguous float64 tensors (P, R, K), (P, R, K, D), (P, R, D), (P, R) beside '
                    'x_trial (P, R, D)', (f, (P, R, K)), (J, (P, R, K, D)), (z, (P, R, D)), (logu, (P, R)))
        self._chk(self._enter() or lib.dgpamd_boxsmc_move(
            self.h, P, R, D, K, _dp(f), _dp(J), _dp(state['par']), _hp(state['par_h']), _dp(state['beta']), _dp(z), _dp(logu),
            float(hmin), float(hmax), float(up), float(down), 1 if adapt else 0, 1 if first else 0, 1 if last else 0,
            _dp(state['work']), _dp(x_trial), _dp(state['x']), _dp(state['ll']), _dp(state['lprior']), _dp(state['h']),
            _dp(state['logr']), _dp(state['status']), _dp(state['n_prop']), _dp(state['n_acc'])))
        return x_trial

    def boxsmc_temper(self, state, x_trial, u, ess_frac=0.5):
        """One tempering step of every draw (dgpamd_boxsmc_temper): from state's ll, x and beta and the uniforms u (P,), a
        float64 device tensor, the step of beta that keeps ESS >= ess_frac R_live; updates beta, dbeta, log_evidence,
        stage_ess, draw_status, anc and running in place and gathers the resampled particles into x_trial (P, R, D)."""
        P, R, D = self._boxsmc_sizes(state, x_trial)
        _f64_shapes('boxsmc: u must be a contiguous float64 tensor (P,)', (u, (P,)))
        self._chk(self._enter() or lib.dgpamd_boxsmc_temper(
            self.h, P, R, D, float(ess_frac), _dp(state['ll']), _dp(state['x']), _dp(u), _dp(state['beta']), _dp(state['dbeta']),
            _dp(state['log_evidence']), _dp(state['stage_ess']), _dp(state['draw_status']), _dp(state['anc']), _dp(x_trial),
            _dp(state['running'])))
        return x_trial

    # the whitening fold of field calibration (csrc/boxsites.hip)
    BOXSITES_MAXT = 256

    def boxsites_plan(self, W, cols):
        """What the folds of one run share (boxsites_fold's W): W (K, T, T), a host array or a device tensor, the whitening
        matrix W[k, t, s] of every output, transposed once into the kernel's layout Wt[k, s, t]; cols, Dt distinct ints, on the
        device and on the host."""
        Wd = W if torch.is_tensor(W) else self.tensor(np.asarray(W, dtype=np.float64))
        if Wd.dim() != 3 or Wd.shape[1] != Wd.shape[2] or Wd.dtype != torch.float64:
            raise ValueError('boxsites: W must be float64 (K, T, T)')
        cols_h = np.ascontiguousarray(np.asarray(cols, dtype=np.int32).reshape(-1))
        return dict(K=int(Wd.shape[0]), T=int(Wd.shape[1]), Wt=Wd.transpose(1, 2).contiguous(), cols_h=cols_h,
                    cols=torch.as_tensor(cols_h, device=self.device) if cols_h.size else None)

    def boxsites_fold(self, f, J, W, cols=None, out=None):
        """(ft (Q, T K), Jt (Q, T K, Dt)) = dgpamd_boxsites_fold: ft[q, t K + k] = sum_{s <= t} W[k, t, s] f[q, s, k] and
        Jt[q, t K + k, d] = sum_{s <= t} W[k, t, s] J[q, s, k, cols[d]], in the order of s, exact zeros of W skipped.  f
        (Q, T, K), J (Q, T, K, Dx): contiguous float64 device tensors; J None: the values alone, Jt None.  W: boxsites_plan's
        dict (cols is then its own), or (K, T, T) with cols beside it -- a plan made for this call.  out: (ft, Jt) to write
        into.  The layouts are those boxmala_step, boxhmc_step and boxsmc_move take as f and J."""
        plan = W if isinstance(W, dict) else self.boxsites_plan(W, [] if cols is None else cols)
        _f64_shapes('boxsites: f must be a contiguous float64 tensor (Q, T, K)', (f, (None, plan['T'], plan['K'])))
        Q, T, K = f.shape
        Dt = 0 if J is None else int(plan['cols_h'].size)
        if J is not None:
            _f64_shapes('boxsites: J must be a contiguous float64 tensor (Q, T, K, Dx)', (J, (Q, T, K, None)))
        Dx = 1 if J is None else int(J.shape[3])
        ft, Jt = (self.empty(Q, T * K), None if J is None else self.empty(Q, T * K, Dt)) if out is None else out
        _f64_shapes('boxsites: out must be contiguous float64 tensors (Q, T K), (Q, T K, Dt)',
                    *([(ft, (Q, T * K))] + ([] if J is None else [(Jt, (Q, T * K, Dt))])))
        self._chk(self._enter() or lib.dgpamd_boxsites_fold(
            self.h, Q, T, K, Dx, Dt, _dp(plan['cols']) if Dt else None, _hp(plan['cols_h']) if Dt else None, _dp(plan['Wt']),
            _dp(f), _dp(J), _dp(ft), _dp(Jt) if Dt else None))
        return ft, Jt

    # subset simulation (csrc/boxsus.hip)
    BOXSUS = dict(ok=0, nan=1, max_stages=2, below_min=3)
    BOXSUS_MAXR = 8192

    def boxsus_state(self, P, R, D, lo, hi, prior_prec=None, prior_mean=None, step=1.0):
        """What one run keeps between its boxsus_move and boxsus_level calls: par, the prior and the box on the device --
        prior_prec (D, None: 0, the uniform prior), prior_mean (D), lo (D), hi (D) -- and par_h, its host copy; per particle
        x (D, Q) particle fastest, score (Q) and moved, status, n_prop, n_acc (Q) int32, Q = P R; per draw prob (ones), level
        (-inf), lam (filled with step), sd (P, D) (zeros: the caller fills it before the first move), nsurv, done,
        draw_status (P) int32, anc (P, R) int32; running (1,) int32."""
        P, R, D = int(P), int(R), int(D)
        if P < 1 or not 1 <= R <= Engine.BOXSUS_MAXR or P * R >= 2 ** 31 or not 1 <= D <= _lib.MAXD:
            raise ValueError('boxsus: need P >= 1, 1 <= R <= %d, P R < 2^31 and 1 <= D <= %d' % (Engine.BOXSUS_MAXR, _lib.MAXD))
        lo, hi = _f64(lo), _f64(hi)
        pv = np.zeros(D) if prior_prec is None else _f64(prior_prec)
        pm = np.zeros(D) if prior_mean is None else _f64(prior_mean)
        if any(a.size != D for a in (lo, hi, pv, pm)):
            raise ValueError('boxsus: lo, hi and the prior must hold D = %d entries' % D)
        par, Q = np.concatenate([pv, pm, lo, hi]), P * R
        i32 = dict(dtype=torch.int32)
        return dict(P=P, R=R, D=D, par_h=par, par=self.tensor(par), x=self.zeros(D, Q), score=self.zeros(Q),
                    moved=self.zeros(Q, **i32), status=self.zeros(Q, **i32), n_prop=self.zeros(Q, **i32),
                    n_acc=self.zeros(Q, **i32), prob=torch.ones(P, dtype=torch.float64, device=self.device),
                    level=torch.full((P,), -np.inf, dtype=torch.float64, device=self.device),
                    lam=torch.full((P,), float(step), dtype=torch.float64, device=self.device), sd=self.zeros(P, D),
                    nsurv=self.zeros(P, **i32), done=self.zeros(P, **i32), draw_status=self.zeros(P, **i32),
                    anc=self.zeros(P, R, **i32), running=self.zeros(1, **i32))

    def _boxsus_sizes(self, state, x_trial):
        return self._pop_sizes(
            'boxsus', 'P, R or D', state, x_trial, lambda P, R, D: state['D'] == D and state['par_h'].size == 4 * D,
            lambda P, R, D, Q: dict(x=Q * D, score=Q, moved=Q, status=Q, n_prop=Q, n_acc=Q, prob=P, level=P, lam=P, sd=P * D, nsurv=P,
                                    done=P, draw_status=P, anc=Q, running=1, par=4 * D))

    def boxsus_move(self, state, f, x_trial, z, logu, threshold, output=0, sign=1.0, first=False, last=False):
        """One call of every particle's modified Metropolis state machine (dgpamd_boxsus_move).  state: boxsus_state's; f
        (P, R, K): the walk's values at x_trial (P, R, D), of which column output is read, score = sign (f - threshold) + 0;
        z, logu (P, R, D): this call's normal draws and logarithms of uniform draws; all contiguous float64 device tensors.
        first: a stage starts -- the state comes from x_trial.  last: the stage ends -- x_trial <- x instead of a proposal.
        x_trial is overwritten with the next points to evaluate."""
        P, R, D = self._boxsus_sizes(state, x_trial)
        if f.dim() != 3:
            raise ValueError('boxsus: f must be (P, R, K)')
        K = f.shape[-1]
        _f64_shapes('boxsus: f, z, logu must be contiguous float64 tensors (P, R, K), (P, R, D), (P, R, D) beside x_trial (P, R, D)',
                    (f, (P, R, K)), (z, (P, R, D)), (logu, (P, R, D)))
        self._chk(self._enter() or lib.dgpamd_boxsus_move(
            self.h, P, R, D, K, int(output), float(sign), float(threshold), _dp(f), _dp(state['par']), _hp(state['par_h']),
            _dp(state['level']), _dp(state['lam']), _dp(state['sd']), _dp(z), _dp(logu), 1 if first else 0, 1 if last else 0,
            _dp(x_trial), _dp(state['x']), _dp(state['score']), _dp(state['moved']), _dp(state['status']), _dp(state['n_prop']),
            _dp(state['n_acc'])))
        return x_trial

    def boxsus_level(self, state, x_trial, n_s, min_prob=1e-12):
        """One level step of every draw (dgpamd_boxsus_level): from state's score and x, the n_s-th largest live score as
        the next level (+0 once it is reached: the draw's final stage), the survivors and their count, prob times their
        share, the ancestors and the survivors' spread sd; updates prob, level, nsurv, done, draw_status, anc, sd and running
        in place and gathers the cloned particles into x_trial (P, R, D)."""
        P, R, D = self._boxsus_sizes(state, x_trial)
        self._chk(self._enter() or lib.dgpamd_boxsus_level(
            self.h, P, R, D, int(n_s), float(min_prob), _dp(state['score']), _dp(state['x']), _dp(state['prob']),
            _dp(state['level']), _dp(state['nsurv']), _dp(state['done']), _dp(state['draw_status']), _dp(state['anc']),
            _dp(x_trial), _dp(state['sd']), _dp(state['running'])))
        return x_trial

    # counter-based random streams (csrc/philox.hip)
    PHILOX = dict(bits=0, uniform=1, log_uniform=2, normal=3)

    @staticmethod
    def philox_key(seed):
        """(key0, key1) of a seed: numpy.random.SeedSequence(seed).generate_state(2, uint64); None draws fresh entropy."""
        k = np.random.SeedSequence(seed).generate_state(2, np.uint64)
        return int(k[0]), int(k[1])

    @staticmethod
    def philox_check(kind, key, stream, c2_first, rounds, P, R, D):
        """philox_fill's refusals, which need no device; (kind number, key0, key1, stream, c2_first, rounds, P, R, D)."""
        if kind not in Engine.PHILOX:
            raise ValueError('philox: kind must be one of %s' % ', '.join(Engine.PHILOX))
        try:
            k0, k1 = (int(k) for k in key)
        except (TypeError, ValueError):
            raise ValueError('philox: key must be two integers in 0 .. 2^64 - 1') from None
        stream, c2_first, rounds, P, R, D = int(stream), int(c2_first), int(rounds), int(P), int(R), int(D)
        if any(not 0 <= v < 2 ** 64 for v in (k0, k1, stream, c2_first)):
            raise ValueError('philox: key, stream and c2_first must lie in 0 .. 2^64 - 1')
        if rounds < 1 or P < 1 or R < 1 or not 1 <= D <= _lib.MAXD:
            raise ValueError('philox: need rounds >= 1, P >= 1, R >= 1 and 1 <= D <= %d' % _lib.MAXD)
        if P >= 2 ** 31 or R >= 2 ** 32 or c2_first + rounds >= 2 ** 64 or rounds * P * R > 2 ** 56:
            raise ValueError('philox: need P < 2^31, R < 2^32, c2_first + rounds < 2^64 and rounds P R <= 2^56')
        return Engine.PHILOX[kind], k0, k1, stream, c2_first, rounds, P, R, D

    def philox_fill(self, kind, key, stream, c2_first, rounds, P, R, D, out=None):
        """(rounds, P, R, D) numbers of one Philox4x64-10 stream, made on the device (dgpamd_philox_fill): entry [i, p, r, e] is
        a pure function of (key, stream, c2_first + i, p, r, e), whatever the shape of the call.  kind: a key of Engine.PHILOX --
        'bits' the raw words (int64), 'uniform' in [0, 1), 'log_uniform', 'normal' (float64).  key: two 64-bit integers
        (philox_key(seed)).  out: a contiguous tensor of that shape and type to fill instead of a new one."""
        args = self.philox_check(kind, key, stream, c2_first, rounds, P, R, D)
        shape, dtype = args[5:], torch.int64 if kind == 'bits' else torch.float64
        if out is None:
            out = self.empty(*shape, dtype=dtype)
        elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != self.device:
            raise ValueError('philox: out must be a contiguous %s device tensor (rounds, P, R, D)' % dtype)
        self._chk(self._enter() or lib.dgpamd_philox_fill(self.h, *args, _dp(out)))
        return out

    # --------------------------------------------------------------- vecchia
    def nn_ordered(self, x, m):
        n, D = x.shape
        m = min(m, n - 1)
        out = self.empty(n, m + 1, dtype=torch.int64)
        self._chk(self._enter() or lib.dgpamd_nn_ordered(self.h, n, D, _dp(x), m, _dp(out)))
        return out

    MATHFN = dict(exp_negated=0, exp_negated_v3=1, exp_negated_tab=2, exp_negated_tab2=3, cos_reduced=4, cos_sin_reduced=5,
                  rsqrt=6, rsqrt_sqrt=7, rcp=8, dlog_matern25=9, dlog_sexp=10, exp_table=11, tri_decode=12)
    _MATHFN_TWO = ('cos_sin_reduced', 'rsqrt_sqrt', 'tri_decode')

    def debug_mathfn(self, fn, a):
        """Testing aid (dgpamd_debug_mathfn): one of the library's own device math functions on every element of the float64 tensor
        `a`, one lane per element.  fn: a key of Engine.MATHFN.  Returns one tensor, or two for the functions with two results."""
        a = a.contiguous()
        out0 = self.empty(a.numel())
        out1 = self.empty(a.numel()) if fn in self._MATHFN_TWO else None
        self._chk(self._enter() or lib.dgpamd_debug_mathfn(self.h, self.MATHFN[fn], a.numel(), _dp(a), _dp(out0), _dp(out1)))
        return out0 if out1 is None else (out0, out1)

    LINKFN = dict(i=0, jd=1, jd0=2, jsep=3, jsep0=4, erfcx=5)

    def debug_linkfn(self, fn, args):
        """Testing aid (dgpamd_debug_linkfn): one of the Matern-2.5 linked-GP factors of csrc/linkfun.hpp on every row
        (X1, X2, m, v, l) of the float64 tensor `args` (count x 5), one lane per row.  fn: a key of Engine.LINKFN."""
        args = args.contiguous()
        assert args.dim() == 2 and args.shape[1] == 5
        out = self.empty(args.shape[0])
        self._chk(self._enter() or lib.dgpamd_debug_linkfn(self.h, self.LINKFN[fn], args.shape[0], _dp(args), _dp(out)))
        return out

    def nn_query(self, q, x, m):
        M, D = q.shape
        n = x.shape[0]
        m = min(m, n)
        out = self.empty(M, m, dtype=torch.int64)
        self._chk(self._enter() or lib.dgpamd_nn_query(self.h, M, n, D, _dp(q), _dp(x), m, _dp(out)))
        return out

    def vecchia_llik(self, kind, X, y, NN, length, nugget, nugget_diag):
        """(quad, logdet) summed over the rows of NN.  NN may be a block of rows of the neighbour array (the rows a rank
        owns, dist.vecchia_rows): X, y and nugget_diag are indexed through its entries, so they stay whole."""
        n, D = NN.shape[0], X.shape[1]
        length = _f64(length)
        out = self.empty(2)
        self._chk(self._enter() or lib.dgpamd_vecchia_llik(self.h, KIND[kind], n, D, NN.shape[1] - 1, _dp(X), _dp(y), _dp(NN), _hp(length),
                                          len(length), float(nugget), _dp(nugget_diag), _dp(out)))
        return out

    def vecchia_llik_batch(self, kind, Xall, y, NN, length, nugget, nugget_diag):
        """vecchia_llik for the B input sets Xall (B, n_points, D) at once: (B, 2) sums, one row launch + one reduction."""
        B, D = Xall.shape[0], Xall.shape[2]
        length = _f64(length)
        out = self.empty(B, 2)
        self._chk(self._enter() or lib.dgpamd_vecchia_llik_batch(self.h, KIND[kind], NN.shape[0], D, NN.shape[1] - 1, _dp(Xall),
                                                                 Xall.stride(0), B, _dp(y), _dp(NN), _hp(length), len(length),
                                                                 float(nugget), _dp(nugget_diag), _dp(out)))
        return out

    def vecchia_nllik(self, kind, X, y, NN, length, nugget, nugget_diag, nugget_est):
        n, D = NN.shape[0], X.shape[1]   # (rows of NN: possibly one rank's block, see vecchia_llik)
        length = _f64(length)
        P = (1 if len(length) == 1 else D) + (1 if nugget_est else 0)
        out = self.empty(2 + 2 * P)
        self._chk(self._enter() or lib.dgpamd_vecchia_nllik(self.h, KIND[kind], n, D, NN.shape[1] - 1, _dp(X), _dp(y), _dp(NN),
                                           _hp(length), len(length), float(nugget), _dp(nugget_diag),
                                           1 if nugget_est else 0, _dp(out)))
        return out, P

    def vecchia_lmatrix(self, kind, X, NN, length, nugget):
        n, D = X.shape
        length = _f64(length)
        out = self.empty(n, NN.shape[1])
        self._chk(self._enter() or lib.dgpamd_vecchia_lmatrix(self.h, KIND[kind], n, D, NN.shape[1] - 1, _dp(X), _dp(NN), _hp(length),
                                             len(length), float(nugget), _dp(out)))
        return out

    def vecchia_post_het(self, kind, X_ord, impNN, scale, length, gamma, y, z):
        """Draw of the mean latent from its exact conditional posterior under a Hetero likelihood, Vecchia form
        (likelihood_class.py:153-182 on vecchia.U_matrix_sp :599-610), in ORDERED coordinates:
        f = -U_l^-T U_ol^T y + U_l^-T z.  X_ord (n x D), impNN (n x (m+1)) int64, gamma / y / z (n), all on the device."""
        import torch
        n, D = X_ord.shape
        mp1 = impNN.shape[1]
        length = _f64(length)
        Lrows, t = self.empty(n, mp1), self.empty(n)
        NNl = torch.empty((n, mp1), dtype=torch.int64, device=X_ord.device)
        info = torch.empty(1, dtype=torch.int32, device=X_ord.device)
        self._chk(self._enter() or lib.dgpamd_vecchia_het_rows(self.h, KIND[kind], n, D, mp1 - 1, _dp(X_ord), _dp(impNN), _hp(length), len(length),
                                              float(scale), _dp(gamma), _dp(y), _dp(Lrows), _dp(NNl), _dp(t), _dp(info)))
        bad = int(info.item())
        if bad:
            raise np.linalg.LinAlgError('Vecchia block of row %d is not positive definite' % (bad - 1))
        return self.vecchia_spsolve(Lrows, NNl, 1.0, z) - self.vecchia_spsolve(Lrows, NNl, 1.0, t)

    def vecchia_spsolve(self, Lmat, NN, inv_sqrt_scale, b):
        n = Lmat.shape[0]
        out = self.empty(n)
        self._chk(self._enter() or lib.dgpamd_vecchia_spsolve(self.h, n, NN.shape[1] - 1, _dp(Lmat), _dp(NN), float(inv_sqrt_scale), _dp(b),
                                             _dp(out)))
        return out

    def vecchia_spsolve_batch(self, Lmat, NN, inv_sqrt_scale, b):
        """Lmat, NN: (nmat, n, m+1); inv_sqrt_scale: nmat floats; b: (nmat, nrhs, n) -> x of the same shape."""
        nmat, n, mp1 = Lmat.shape
        nrhs = b.shape[1]
        out = self.empty(nmat, nrhs, n)
        sc = self.tensor(np.asarray(inv_sqrt_scale, dtype=np.float64))
        self._chk(self._enter() or lib.dgpamd_vecchia_spsolve_batch(self.h, n, mp1 - 1, nmat, nrhs, _dp(Lmat), _dp(NN), _dp(sc), _dp(b), _dp(out)))
        return out

    def vecchia_levels(self, NN):
        """Level schedule of the sparse forward substitution for the neighbour arrays NN (nmat, n, m+1) or (n, m+1): an int32
        device tensor for vecchia_spsolve_levels; depends on NN only (build once per ordering)."""
        if NN.dim() == 2:
            NN = NN.unsqueeze(0)
        nmat, n, mp1 = NN.shape
        sched = torch.empty(int(lib.dgpamd_vecchia_levels_bytes(n, nmat)) // 4, dtype=torch.int32, device=self.device)
        self._chk(self._enter() or lib.dgpamd_vecchia_levels(self.h, n, mp1 - 1, nmat, _dp(NN.contiguous()), _dp(sched)))
        return sched

    def vecchia_spsolve_levels(self, Lmat, NN, inv_sqrt_scale, b, sched):
        """vecchia_spsolve_batch on a level schedule (vecchia_levels of the same NN)."""
        nmat, n, mp1 = Lmat.shape
        nrhs = b.shape[1]
        out = self.empty(nmat, nrhs, n)
        sc = self.tensor(np.asarray(inv_sqrt_scale, dtype=np.float64))
        self._chk(self._enter() or lib.dgpamd_vecchia_spsolve_levels(self.h, n, mp1 - 1, nmat, nrhs, _dp(Lmat), _dp(NN), _dp(sc), _dp(b), _dp(out),
                                                                   _dp(sched)))
        return out

    def vpaths_nn(self, q, x, m, group=None):
        """Conditioning sets of Vecchia sample paths (dgpamd_vpaths_nn): q (P, M, D) the paths' scaled test rows in their
        order, x (G, n, D) scaled training sets, group None or int32 device (P,).  Returns (P, M, m) int64 combined indices."""
        P, M, D = q.shape
        n = x.shape[-2]
        out = self.empty(P, M, m, dtype=torch.int64)
        self._chk(self._enter() or lib.dgpamd_vpaths_nn(self.h, P, M, n, D, int(m), _dp(q), _dp(x), _dp(group), _dp(out)))
        return out

    def vpaths_rows(self, kind, q, x, NN, y, scale, nugget, omega=None, group=None, jitter=0.0):
        """Rows of the Vecchia sample-path substitution (dgpamd_vpaths_rows): q (P, M, D), x (G, n, D) scaled as for
        vpaths_nn, NN its result, y (G, nrhs, n) right-hand sides.  Returns Lrows (P, M, m+1), NNl (P, M, m+1), t (P, nrhs, M),
        sd (P, M) and the device info word."""
        P, M, D = q.shape
        n, m, nrhs = x.shape[-2], NN.shape[2], y.shape[-2]
        Lrows, t, sd = self.empty(P, M, m + 1), self.empty(P, nrhs, M), self.empty(P, M)
        NNl = self.empty(P, M, m + 1, dtype=torch.int64)
        info = self.empty(1, dtype=torch.int32)
        self._chk(self._enter() or lib.dgpamd_vpaths_rows(self.h, KIND[kind], P, M, n, D, m, nrhs, _dp(q), _dp(x), _dp(group), _dp(NN),
                                                          _dp(omega), _dp(y), float(scale), float(nugget), float(jitter), _dp(Lrows),
                                                          _dp(NNl), _dp(t), _dp(sd), _dp(info)))
        return Lrows, NNl, t, sd, info

    def vpathfun_update(self, kind, x, w, NN, r, prior, scale, nugget, jitters, omega=None, out=None):
        """The locally conditioned pathwise update of function-valued draws (dgpamd_vpathfun_update):
            out = sqrt(scale) (prior + sum_j b_j r[N_j]),  b = A_N^-1 c(W_N, x),
        N the row's neighbours NN (rows, pm) int64 (nn_query's: valid first, -1 padded), A_N their correlation block with
        diagonal 1 + jitter + nugget * omega_j.  x and w (n, D) are coordinates divided by the lengthscales.
        Shared rows: x (M, D), r (n, P) neighbour-major, prior (M, P); returns out (M, P) -- path fastest, the layout the
        kernel loads and stores coalesced.  Per-path rows: x (P, M, D), r (P, n), prior (P, M); returns out (P, M).
        jitters: the ladder tried row by row (first entry normally 0).  Returns (out, info): info 2 device int32, [0] rows
        that needed a later rung, [1] 1 + the smallest row (p * M + i for per-path rows) that failed them all, or -1."""
        n, D = w.shape
        shared = x.dim() == 2
        if shared:
            M, P = x.shape[0], r.shape[1]
            R, rows_per_path, shape = M, 0, (M, P)
            assert r.shape == (n, P)
        else:
            P, M = x.shape[:2]
            R, rows_per_path, shape = P * M, M, (P, M)
            assert r.shape == (P, n)
        assert x.shape[-1] == D and NN.shape[0] == R and NN.dim() == 2 and NN.dtype == torch.int64 and prior.shape == shape
        assert omega is None or omega.shape == (n,)
        for t in (x, w, NN, r, prior, omega):
            assert t is None or (t.is_contiguous() and (t is NN or t.dtype == torch.float64))
        jit = _f64(jitters)
        out = self.empty(*shape) if out is None else out
        assert out.shape == shape and out.is_contiguous()
        info = self.empty(2, dtype=torch.int32)
        self._chk(self._enter() or lib.dgpamd_vpathfun_update(self.h, KIND[kind], R, n, D, NN.shape[1], P, rows_per_path, _dp(x), _dp(w),
                                                              _dp(NN), _dp(omega), _dp(r), _dp(prior), float(scale), float(nugget),
                                                              _hp(jit), len(jit), _dp(out), _dp(info)))
        return out, info

    def vecchia_gp(self, kind, x, w, NN, y, scale, length, nugget, nugget_diag):
        M, D = x.shape
        length = _f64(length)
        mean, var = self.empty(M), self.empty(M)
        self._chk(self._enter() or lib.dgpamd_vecchia_gp(self.h, KIND[kind], M, w.shape[0], D, NN.shape[1], _dp(x), _dp(w), _dp(NN), _dp(y),
                                        float(scale), _hp(length), len(length), float(nugget), _dp(nugget_diag),
                                        _dp(mean), _dp(var)))
        return mean, var

    def vecchia_linkgp(self, kind, m, v, z, w1, wg, NN, y, scale, length, nugget, nugget_diag):
        M, Dw = m.shape
        Dz = 0 if z is None else z.shape[1]
        length = _f64(length)
        mean, var = self.empty(M), self.empty(M)
        self._chk(self._enter() or lib.dgpamd_vecchia_linkgp(self.h, KIND[kind], M, w1.shape[0], Dw, Dz, NN.shape[1], _dp(m), _dp(v), _dp(z),
                                            _dp(w1), _dp(wg), _dp(NN), _dp(y), float(scale), _hp(length), len(length),
                                            float(nugget), _dp(nugget_diag), _dp(mean), _dp(var)))
        return mean, var


_default = {}


def default_engine(device=None):
    """Process-wide engine for `device` (LOCAL_RANK-aware default)."""
    import os
    if device is None:
        device = int(os.environ.get('LOCAL_RANK', '0'))
    if device not in _default:
        _default[device] = Engine(device)
    return _default[device]


class _LlikPlan:
    """Arguments of dgpamd_llik_batch kept alive between the rounds of a lock-step M-step."""

    def __init__(self, eng, n, specs):
        self.e, self.n, self.B = eng, int(n), len(specs)
        B, Np = self.B, eng.padded_dim(n)
        self.keep = specs                      # tensors stay referenced
        self.nodes = (_lib.Node * B)()
        self.lengths = []
        self.P = []
        for b, sp in enumerate(specs):
            nd = self.nodes[b]
            Xl, Xg = sp['Xloc'], sp['Xglob']
            nd.kind = KIND[sp['kind']]
            nd.Dl, nd.Dg = Xl.shape[1], 0 if Xg is None else Xg.shape[1]
            nd.nlen, nd.nugget_est, nd.ldloc = int(sp['nlen']), 1 if sp['nugget_est'] else 0, Xl.shape[1]
            nd.Xloc, nd.colmap, nd.Xglob = Xl.data_ptr(), None, None if Xg is None else Xg.data_ptr()
            length = np.ones(nd.nlen)
            self.lengths.append(length)
            nd.length = length.ctypes.data
            nd.W = None if sp['W'] is None else sp['W'].data_ptr()
            nd.y = sp['y'].data_ptr()
            self.P.append((1 if nd.nlen == 1 else nd.Dl + nd.Dg) + nd.nugget_est)
        self.stride_out = 3 + 2 * max(self.P)
        self.A = eng.workspace(('mstepA', n), B * Np * Np * 8)
        self.Ainv = eng.workspace(('mstepAinv', n), B * Np * Np * 8)
        self.T = eng.workspace(('mstepT', n), B * Np * Np * 8)
        self.work = eng.potrf_workspace(n, B)
        self.gwork = eng.workspace(('gradB', n, max(self.P), B), B * lib.dgpamd_grad_workspace(n, max(self.P)))
        self.dev_out = eng.empty(B * (self.stride_out + 2))
        self.host = np.zeros((B, self.stride_out))
        self.stride_a = Np * Np

    def set(self, b, length, nugget):
        self.lengths[b][:] = length
        self.nodes[b].nugget = float(nugget)

    def factor_view(self, r):
        """The augmented buffer of row r of the LAST run() as an (Np, Np) float64 tensor: after the sweep its lower tiles
        hold the Cholesky factor of that node's K (rows < n), exactly what dgpamd_potrf leaves."""
        Np = self.e.padded_dim(self.n)
        return self.A[r * self.stride_a * 8:(r + 1) * self.stride_a * 8].view(torch.float64).view(Np, Np)

    def launch(self, idx):
        """First half of run(): everything queued on the device (dgpamd_llik_batch_launch); wait(token) returns the results."""
        e = self.e
        if len(idx) == self.B:
            nodes, B = self.nodes, self.B
        else:
            B = len(idx)
            nodes = (_lib.Node * B)(*[self.nodes[i] for i in idx])
        e._chk(e._enter() or lib.dgpamd_llik_batch_launch(e.h, self.n, B, nodes, _dp(self.A), _dp(self.T), _dp(self.Ainv), self.stride_a, _dp(self.work),
                                                          _dp(self.gwork), _dp(self.dev_out), self.stride_out))
        return (list(idx), nodes)   # (the node array stays alive until the wait)

    def wait(self, token):
        idx = token[0]
        e = self.e
        host = self.host[:len(idx)]
        e._chk(e._enter() or lib.dgpamd_llik_batch_wait(e.h, host.ctypes.data_as(C.c_void_p)))
        out = {}
        for r, i in enumerate(idx):
            P = self.P[i]
            out[i] = np.concatenate((host[r, :2], host[r, 3:3 + 2 * P], host[r, 2:3]))
        return out

    def run(self, idx):
        """Evaluate the nodes listed in idx (positions in the plan); returns {position: host vector
        [logdet, y'K^-1y, tr.., quad.., info]} in kernel._llik_device's layout."""
        e = self.e
        if len(idx) == self.B:
            nodes, B = self.nodes, self.B
        else:
            B = len(idx)
            nodes = (_lib.Node * B)(*[self.nodes[i] for i in idx])
        host = self.host[:B]
        e._chk(e._enter() or lib.dgpamd_llik_batch(e.h, self.n, B, nodes, _dp(self.A), _dp(self.T), _dp(self.Ainv), self.stride_a, _dp(self.work),
                                     _dp(self.gwork), _dp(self.dev_out), host.ctypes.data_as(C.c_void_p), self.stride_out))
        out = {}
        for r, i in enumerate(idx):
            P = self.P[i]
            out[i] = np.concatenate((host[r, :2], host[r, 3:3 + 2 * P], host[r, 2:3]))
        return out


def cell_order(W, leaf=16, block=64):
    """A permutation of the rows of W (n x D training inputs of a linked node) that groups them by cells: recursive
    splits at an order statistic of one coordinate (the coordinates in turn), every part a multiple of `block` rows while it
    is larger than a block and of `leaf` rows below, down to `leaf` rows.  Rows 16 a .. 16 a + 15 of the permuted array are
    then a cell, and two cells that were separated by a split in coordinate k satisfy max x_k <= min x_k one way round.  The
    Matern pair kernel (linkgp_Jsep_kernel) needs one of its two record products for such a (sub-tile, coordinate) and both
    for the others; any order gives the same predictions (functions.py:453-494 sums over all pairs)."""
    W = np.asarray(W, dtype=float)
    n, D = W.shape
    out = []
    stack = [(np.arange(n), 0)]
    while stack:
        idx, depth = stack.pop()
        m = len(idx)
        if m <= leaf:
            out.append(idx)
            continue
        unit = block if m > block else leaf
        left = unit * max(1, int(round(m / (2.0 * unit))))
        if left >= m:
            left = m - (m % unit or unit)
        k = depth % D
        o = idx[np.argsort(W[idx, k], kind='stable')]
        stack.append((o[left:], depth + 1))   # (popped after the left part: the output keeps left before right)
        stack.append((o[:left], depth + 1))
    return np.concatenate(out)


LIK_KIND = {'Poisson': 1, 'NegBin': 2, 'ZIP': 3, 'ZINB': 4, 'logit': 5, 'probit': 6, 'robustmax': 7, 'softmax': 8}


def _fill_lik_node(nd, colmap, lik, M):
    """dgpamd_node fields of a likelihood node (include/dgp_amd.h); returns what must stay alive with the struct."""
    colmap = np.ascontiguousarray(np.asarray(colmap, dtype=np.int32))
    nd.kind, nd.Dl, nd.Dg, nd.nlen, nd.ldloc = 0, len(colmap), 0, 0, M
    nd.colmap = colmap.ctypes.data
    nd.y = lik['y'].data_ptr()
    nd.lik_kind, nd.lik_classes = LIK_KIND[lik['kind']], int(lik.get('classes') or 0)
    nd.lik_nobs = int(lik['y'].numel())
    nd.lik_rep = None if lik.get('rep') is None else lik['rep'].data_ptr()
    nd.lik_par = float(lik.get('par') or 0.0)
    return (colmap, lik['y'], lik.get('rep'))


def _fill_gp_node(nd, kind, colmap, Xglob, length, nugget, W, y, M):
    """dgpamd_node fields of a GP node that reads its local inputs through `colmap` from an (n, M) latent block
    (include/dgp_amd.h); returns what must stay alive with the struct."""
    colmap = np.ascontiguousarray(np.asarray(colmap, dtype=np.int32))
    length = np.ascontiguousarray(np.asarray(length, dtype=np.float64))
    nd.kind, nd.Dl, nd.Dg = KIND[kind], len(colmap), 0 if Xglob is None else Xglob.shape[1]
    nd.nlen, nd.nugget_est, nd.ldloc = len(length), 0, M
    nd.Xloc, nd.colmap = None, colmap.ctypes.data
    nd.Xglob = None if Xglob is None else Xglob.data_ptr()
    nd.length, nd.nugget = length.ctypes.data, float(nugget)
    nd.W = None if W is None else W.data_ptr()
    nd.y = y.data_ptr()
    return (colmap, length, Xglob, W, y)


class _EssQueue:
    """Several elliptical-slice updates of one latent block queued without host synchronisation (dgpamd_ess_queue):
    node structs, scratch and the device state are kept alive here; fetch() is the one synchronisation.  Several queues
    (the layers of a deeper model) can share one device state and one uploaded uniform stream: share_with()."""
    STATE = 16
    FIELDS = ('theta', 'lo', 'hi', 'pending', 'cursor', 'status', 'info', 'll', 'log_y', 'proposals', 'batches', 'updates')

    def __init__(self, eng, n, M, nodes, batch):
        """nodes: list of dicts {kind, colmap, Xglob, length, nugget, W, y} -- the GP nodes of the layer above; a Vecchia
        node adds vecch = dict(ord, nn, nd, y): device tensors (ordering, neighbour array, ordered nugget weights, ordered
        outputs; kernel_class.py:494-509)."""
        self.e, self.n, self.M, self.batch = eng, int(n), int(M), int(batch)
        Np = eng.padded_dim(n)
        self.keep = []
        arr = (_lib.Node * len(nodes))()
        dense, Dv = False, 0
        nodes = list(nodes)
        for i, d in enumerate(nodes):
            if d.get('lik') is not None:   # a likelihood node: dict(kind, y, rep, classes, par) + colmap
                self.keep.append(_fill_lik_node(arr[i], d['colmap'], d['lik'], M))
                continue
            nd = arr[i]
            v = d.get('vecch')
            self.keep += [_fill_gp_node(nd, d['kind'], d['colmap'], d['Xglob'], d['length'], d['nugget'], d['W'], d['y'], M), v]
            if v is not None:
                nd.vecch_ord, nd.vecch_nn = v['ord'].data_ptr(), v['nn'].data_ptr()
                nd.vecch_nd, nd.vecch_y = v['nd'].data_ptr(), v['y'].data_ptr()
                nd.vecch_m = int(v['nn'].shape[1]) - 1
                if v.get('rows') is not None:   # this rank's block of rows (dist.split_training(rows=True)): the sums are all-reduced
                    nd.vecch_row0, nd.vecch_rows = int(v['rows'][0]), int(v['rows'][1] - v['rows'][0])
                    eng.use_dist_reduce()
                Dv = max(Dv, nd.Dl + nd.Dg)
            else:
                dense = True
        self.nodes, self.nnodes = arr, len(nodes)
        self.FP = eng.workspace(('essFP', n, M, batch), batch * n * M * 8)
        self.A = eng.workspace(('essA', n, batch), batch * Np * Np * 8) if dense else None
        self.work = eng.potrf_workspace(n, batch) if dense else None
        self.vwork = eng.workspace(('essV', n, Dv, batch), int(lib.dgpamd_ess_queue_vwork(n, Dv, batch))) if Dv else None
        self.scratch = eng.workspace(('essQ',), int(lib.dgpamd_ess_queue_scratch()))
        self.state = eng.empty(self.STATE)
        self.udev = None

    def share_with(self, other):
        """Continue `other`'s queue: the same device state and the same uploaded uniforms."""
        self.state, self.udev = other.state, other.udev

    def upload_uniforms(self, uniforms):
        e = self.e
        if self.udev is None or self.udev[0] is not uniforms:
            us = np.ascontiguousarray(np.asarray(uniforms, dtype=np.float64))
            with np.errstate(divide='ignore'):
                both = np.concatenate((us, np.log(us)))
            self.udev = (uniforms, e.tensor(both), len(us))

    def reset_state(self, cursor=0, ll=None):
        """A fresh device state (status, counters, info zero; the uniform cursor and the cached log-likelihood as given).  What
        queue(fresh=True) does first; callers that queue other work between the reset and the first update -- a deeper layer's
        prior factorisation, whose info word note_info() folds into this state -- reset here and queue with fresh=False."""
        st0 = np.zeros(self.STATE)
        st0[4], st0[7] = cursor, 0.0 if ll is None else ll
        self.state.copy_(self.e.tensor(st0))

    def queue(self, F, NU, scales, uniforms, cursor, ll, compute_ll0, batch_next, max_batches, fresh=True):
        """Queue NU.shape[0] updates (NU: (nupd, n, M) device tensor).  uniforms: the sampler's upcoming uniforms (host);
        cursor: how many of them earlier queues of this I-step have consumed.  fresh=False: the device state is the one an
        earlier queue() of this I-step left (cursor, status and counters carry on; `cursor` and `ll` are ignored)."""
        e = self.e
        self.upload_uniforms(uniforms)
        ud, nuni = self.udev[1], self.udev[2]
        if fresh:
            self.reset_state(cursor, ll)
        sc = np.ascontiguousarray(np.asarray(scales, dtype=np.float64))
        e._chk(e._enter() or lib.dgpamd_ess_queue(e.h, self.n, self.M, _dp(F), _dp(NU), int(NU.shape[0]), C.cast(self.nodes, C.c_void_p),
                                    sc.ctypes.data_as(C.c_void_p), self.nnodes, _dp(self.state), _dp(ud), _dp(ud[nuni:]), nuni,
                                    self.batch, int(batch_next) if batch_next else self.batch, int(max_batches),
                                    int(compute_ll0), _dp(self.FP), _dp(self.A), _dp(self.work), _dp(self.scratch),
                                    _dp(self.vwork)))

    def resume_state(self, st, ll=None):
        """The device state for a queue that CONTINUES the update an earlier one left open (status 3 / 1): angle, bracket, pending flag and threshold as
        fetched (`st`: fetch()'s dict), status and counters zero, the cursor at the start of the uniforms the next queue() uploads."""
        st0 = np.zeros(self.STATE)
        st0[0], st0[1], st0[2], st0[3] = st['theta'], st['lo'], st['hi'], st['pending']
        st0[7] = st['ll'] if ll is None else ll
        st0[8] = st['log_y']
        self.state.copy_(self.e.tensor(st0))

    def note_info(self, info):
        """A factorisation queued between two updates (a deeper layer's prior factors): non-zero info stops the queue."""
        e = self.e
        e._chk(e._enter() or lib.dgpamd_ess_queue_note_info(e.h, _dp(self.state), _dp(info), int(info.numel())))

    def fetch(self):
        """The ONE synchronisation: the device state as a dict."""
        v = self.e.fetch(self.state)
        return dict(zip(self.FIELDS, v[:len(self.FIELDS)]))


class _EssPlan:
    """One elliptical-slice update per call: dgpamd_ess_update with its scratch buffers kept alive."""

    def __init__(self, eng, n, M, kind, colmap, Xglob, length, nugget, W, y, batch):
        self.e, self.n, self.M, self.batch = eng, int(n), int(M), int(batch)
        Np = eng.padded_dim(n)
        self.node = _lib.Node()
        self.keep = _fill_gp_node(self.node, kind, colmap, Xglob, length, nugget, W, y, M)
        self.FP = eng.workspace(('essFP', n, M, batch), batch * n * M * 8)
        self.A = eng.workspace(('essA', n, batch), batch * Np * Np * 8)
        self.work = eng.potrf_workspace(n, batch)
        self.ll = eng.empty(batch)
        self.info = eng.empty(batch, dtype=torch.int32)
        self.state = np.zeros(4)
        self.out = np.zeros(6)

    def run(self, F, NU, scale, log_y, theta, lo, hi, pending, uniforms, batch_next):
        """Returns (status, consumed, proposals, batches, ll, info, theta, lo, hi, pending)."""
        e = self.e
        us = np.ascontiguousarray(np.asarray(uniforms, dtype=np.float64))
        self.state[:] = (theta, lo, hi, 1.0 if pending else 0.0)
        e._chk(e._enter() or lib.dgpamd_ess_update(e.h, self.n, self.M, _dp(F), _dp(NU), C.byref(self.node), float(scale), float(log_y),
                                     self.state.ctypes.data_as(C.c_void_p), us.ctypes.data_as(C.c_void_p), len(us),
                                     self.batch, int(batch_next) if batch_next else self.batch, _dp(self.FP), _dp(self.A),
                                     _dp(self.work), _dp(self.ll), _dp(self.info), self.out.ctypes.data_as(C.c_void_p)))
        o, st = self.out, self.state
        return int(o[0]), int(o[1]), int(o[2]), int(o[3]), float(o[4]), int(o[5]), st[0], st[1], st[2], bool(st[3])
