// The factorisation as one launch per 64-column block step (potrf mode 0): potrf_step_kernel, its task tables on the
// device and its launches.  The tables are built by potrf_plan.hpp's build_tasks; the tile helpers are chol_tile.hpp's.
// Compiled by potrf.hip, in one unit with potrf_mega.hpp (see there).
#pragma once
#include "chol_tile.hpp"

static_assert(sizeof(Task4) == sizeof(int4) && alignof(Task4) == alignof(int4), "Task4 is uploaded as int4");
static_assert(offsetof(Task4, x) == offsetof(int4, x) && offsetof(Task4, y) == offsetof(int4, y) &&
              offsetof(Task4, z) == offsetof(int4, z) && offsetof(Task4, w) == offsetof(int4, w), "Task4 is uploaded as int4");

// ----------------------------------------------------------------------------
// diagonal block: Cholesky + inverse of the factor (diagfac.hpp)
// ----------------------------------------------------------------------------
// logdet / info of the block just factored (wave 0 knows about failed pivots; the factor's last barrier made the
// pivots visible).  Kept out of diag_factor so that the chain publishes its block BEFORE this reduction.
__device__ __forceinline__ void diag_logdet(DiagShared &sh, int ncol, int k, int b, int bad, double *logdet, int32_t *info) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        const double pv = sh.piv[tid];
        double v = (tid < ncol && pv > 0.0) ? log(pv) : 0.0;   // (a failed pivot is reported through info)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (tid == 0) {
            // (device-scope accesses: the words are read-modified by the chain workgroups of consecutive launches, which run
            //  on whatever XCD the dispatcher picks, and the workspace address they live at holds other data -- diagonal-block
            //  inverses -- under another batch size's layout: no per-XCD L2 line of an earlier use may serve them)
            const double ld0 = k == 0 ? 0.0 : __hip_atomic_load(logdet + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(logdet + b, ld0 + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int inf = k == 0 ? 0 : __hip_atomic_load(info + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (bad && inf == 0) inf = k * 64 + bad;
            __hip_atomic_store(info + b, inf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ----------------------------------------------------------------------------
// One block step k of the factorisation as ONE launch, driven by a TASK TABLE built on the host (one task per
// workgroup and matrix, in urgency = dispatch order).  A task is a 64x64 tile update
//      C = (first ? 0 : C) +/- sum_{kb0 <= kb < kb0+nkb}  L[li][kb] R[ri][kb]^T          (buffers A / T / S)
// followed by one of
//   STORE   (bulk)   store the tile;
//   CHAIN            factor the diagonal tile (diag_factor) and publish the block's inverse W_k with an agent-scope
//                    release (MI355X_MICROARCH.md hand-off recipe);
//   SOLVE   (panel)  wait for that flag (acquire, bounded spin), tile <- tile * W_k^T  -- the explicit inverse of the
//                    diagonal block turns every triangular solve into an MFMA GEMM;
//   TDIAG            wait, write W_k^T (the diagonal block of L^-T).
// Plain factorisation (buffer A): column k = chain + panel tasks applying panel k-1; the bulk is LAZY -- tiles of the
// columns k+1, k+1+LAZY, ... take LAZY = 4 panels (256 pivots) per visit, so C is read/written once per 256 pivots
// while the serial chain still applies a single panel.
// Fused inverse (dgpamd_potrf_inv): the identity rides along as n extra rows (buffer T, only its non-zero tiles
// exist) with a zero corner (buffer S).  The same right-looking sweep then leaves T = L^-T and the Schur
// complement of K in [[K, I], [I, 0]], i.e. S = K^-1 (accumulated with a + sign), and column n of T = -K^-1 y:
// what potri (TRTRI + LAUUM) computes in ~13 more latency-bound launches becomes bulk work in the shadow of the
// pivot chain.  T tiles follow the same lazy rule as A's; S tile (q, q') is visited by the launches
// k = q+2, q+4, ... (two panels each) and by two tail launches.
// CU guard: with two workgroups per CU, workgroups i and i + 256 of a launch share a CU (measured, tools/ubench/
// hwid.hip).  The pivot chain is issue- and LDS-bound and a bulk workgroup beside it slows it by ~40 %, so workgroups
// 256 .. 256+batch-1 are placeholders that sleep until "their" chain has published its block (potrf_inv at B = 3:
// 1.21 -> 1.00 ms).  They hold no task, check through HW_ID / XCC_ID that they really are on the chain's CU, and
// leave at once otherwise.
// Deadlock freedom: only SOLVE / TDIAG workgroups and the placeholders wait, and only for the chain workgroup of the SAME launch, which
// has a lower block index (dispatched first) and never waits itself.  The spin is bounded (info = -1).
// ----------------------------------------------------------------------------
struct StepArgs {
    double *buf[3];   // A (Np x Np, K with the right-hand sides as extra rows), T (L^-T), S (K^-1)
    double *ws;
    int64_t ld, stride_a, stride_ws, n;
    int nbk, k, batch;
    const int4 *tasks;   // this launch's tasks
    int nhead, npanel, lead;   // task order in the table: head (chain, tdiag), panel (solve), bulk; the panel workgroups
                               // are dispatched after the first `lead` bulk tasks (they only wait: no slot hogging)
    int guard, nph;      // guard > 0: workgroups m * guard .. m * guard + batch - 1 (guard = number of CUs, m = 1 .. nph) are
                         // placeholders that keep the chain workgroups' CUs to themselves (nph + 1 workgroups fit a CU)
    double *logdet;
    int32_t *info;
    int32_t *flags;
    long long *trace;
};
#define STAMP(slot)                                                                       \
    do {                                                                                  \
        if (g.trace && b == 0 && tid == 0) g.trace[16 * g.k + (slot)] = wall_clock64();   \
    } while (0)

__global__ __launch_bounds__(256, 2) void potrf_step_kernel(StepArgs g) {
    __shared__ double tiles[2 * 64 * LDM];   // As | Bs
    double *As = tiles, *Bs = tiles + 64 * LDM;
    // the diagonal factor's LDS lives in Bs (idle while a chain workgroup factors): 35 KB per workgroup, four per CU
    static_assert(sizeof(DiagShared) <= 64 * LDM * sizeof(double), "DiagShared must fit the B staging tile");
    DiagShared &sh = *reinterpret_cast<DiagShared *>(Bs);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int crow = 16 * wave + (lane >> 4), ccol = lane & 15;
    const int k = g.k, batch = g.batch;
    int32_t *cukey = g.flags + DGPAMD_MAXB;   // per matrix: (launch + 1) << 16 | CU key of its chain workgroup
    int bidx = blockIdx.x;
    if (g.guard && bidx >= g.guard) {
        // The pivot chain is issue- and LDS-bound: a bulk workgroup on the same CU slows it by ~40 % (measured).  With nph + 1
        // workgroups per CU, workgroups m * (number of CUs) + b (m = 1 .. nph) land beside chain workgroup b: they are placeholders
        // that sleep until that chain has published its block, so the slots are taken and the chain has the CU to itself.  (If
        // the hardware placed one elsewhere it leaves at once.)
        const int row = bidx / g.guard, pos = bidx - row * g.guard;
        if (row <= g.nph && pos < batch) {
            if (tid == 0) {
                const int c = pos, tag = (k + 1) << 16;
                int key = 0, spins = 0;
                while (((key = __hip_atomic_load(&cukey[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 16) != k + 1 &&
                       ++spins < 64)
                    __builtin_amdgcn_s_sleep(2);
                if (key == (tag | cu_key())) {
                    spins = 0;
                    while (__hip_atomic_load(&g.flags[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < k + 1 && ++spins < (1 << 20))
                        __builtin_amdgcn_s_sleep(16);
                }
            }
            return;
        }
        bidx -= batch * (row <= g.nph ? row : g.nph);   // placeholders of this and the earlier rows
    }
    const int b = bidx % batch;
    int slot = bidx / batch;
    if (slot >= g.nhead) {
        if (slot < g.nhead + g.lead) slot += g.npanel;                      // one of the first bulk tasks
        else if (slot < g.nhead + g.lead + g.npanel) slot -= g.lead;        // a panel task
    }
    const int4 tk = g.tasks[slot];
    // debug (dgpamd_debug_trace): per-workgroup start / end / (task kind, panels, CU) of the launch named in trace[4095]
    long long *wtr = (g.trace && tid == 0 && g.trace[4095] == k) ? g.trace + 4096 + 4 * (int64_t)blockIdx.x : nullptr;
    if (wtr) {
        wtr[0] = wall_clock64();
        wtr[2] = task_post(tk.x) | (task_hi(tk.w) << 8) | ((long long)cu_key() << 16);
    }
    const int post = task_post(tk.x), first = task_first(tk.x), plus = task_plus(tk.x), mask_last = task_mask_last(tk.x);
    const int bufC = task_bufC(tk.x), bufL = task_bufL(tk.x), bufR = task_bufR(tk.x);
    const int ci = task_lo(tk.y), cj = task_hi(tk.y), li = task_lo(tk.z), ri = task_hi(tk.z);
    const int kb0 = task_lo(tk.w), nkb = task_hi(tk.w);
    const int64_t ld = g.ld, mo = (int64_t)b * g.stride_a;
    const int64_t rem_last = g.n - (int64_t)(g.nbk - 1) * 64;
    const int ncol_last = rem_last > 0 ? (int)rem_last : 0;   // pivots of the last block (the rest are carried rows)
    double *C = g.buf[bufC] + mo + ((int64_t)ci * 64) * ld + (int64_t)cj * 64;
    double *Wk = g.ws + (int64_t)b * g.stride_ws + (int64_t)k * 4096;

    if (post == T_TDIAG) {   // T[k][k] = W_k^T, rows of the carried right-hand sides zeroed
        wg_wait_acquire(g.flags + b, k + 1, g.info + b, tid);
        const int nrow = (k == g.nbk - 1) ? ncol_last : 64;
        for (int idx = tid; idx < 4096; idx += 256) tiles[(idx >> 6) * 65 + (idx & 63)] = Wk[idx];
        __syncthreads();
        for (int idx = tid; idx < 4096; idx += 256) {
            const int r = idx >> 6, c = idx & 63;
            C[(int64_t)r * ld + c] = r < nrow ? tiles[c * 65 + r] : 0.0;
        }
        return;
    }
    Tile64 acc;
    if (post == T_CHAIN) {
        STAMP(0);
        __builtin_amdgcn_s_setprio(3);
        if (g.guard && tid == 0)
            __hip_atomic_store(&cukey[b], ((k + 1) << 16) | cu_key(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (post == T_CHAIN) {
        if (nkb == 1)
            diag_update_cb(acc.v, C, g.buf[bufL] + mo + ((int64_t)li * 64) * ld + (int64_t)kb0 * 64, ld, As, Bs, tid, wave, lane);
        else {
            load_cb_lower(acc.v, C, ld, wave, lane, Bs);
            __syncthreads();   // (the factor's LDS lives in Bs as well: every wave is done with its transposition scratch)
        }
    } else
        tile_update(acc.v, first ? nullptr : C, g.buf[bufL] + mo + ((int64_t)li * 64) * ld + (int64_t)kb0 * 64,
                    g.buf[bufR] + mo + ((int64_t)ri * 64) * ld + (int64_t)kb0 * 64, ld, nkb, plus ? 1.0 : -1.0,
                    mask_last ? g.nbk - 1 - kb0 : -1, ncol_last, As, Bs, tid, wave, lane);
    if (post == T_STORE) {
        store_acc(acc.v, C, ld, crow, ccol);
        if (wtr) wtr[1] = wall_clock64();
        return;
    }
    if (post == T_CHAIN) {
        STAMP(1);
        const int64_t rem = g.n - (int64_t)k * 64;
        const int ncol = rem >= 64 ? 64 : (rem > 0 ? (int)rem : 0);
        Tile64 winv;
        const int bad = diag_factor(acc, winv, sh, ncol, (g.trace && b == 0) ? g.trace + 1024 + 16 * k : nullptr);
        diag_store_inverse<false>(winv, Wk);
        STAMP(2);
        wg_release_store(g.flags + b, k + 1, tid);   // the panel can start: it needs W_k only
        STAMP(3);
        diag_store_factor(acc, C, ld, ncol);         // the factor's own tile and the log-determinant are nobody's input
        diag_logdet(sh, ncol, k, b, bad, g.logdet, g.info);
        if (wtr) wtr[1] = wall_clock64();
        return;
    }
    // T_SOLVE: wait for W_k, then tile <- tile * W_k^T
    const bool stamp = (bufC == BUF_A && ci == k + 1);
    if (stamp) STAMP(8);
    wg_wait_acquire(g.flags + b, k + 1, g.info + b, tid);
    if (stamp) STAMP(9);
    d4 out[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) out[t] = (d4){0.0, 0.0, 0.0, 0.0};
    mul_acc_bt(out, acc.v, Wk, 64, As, Bs, tid, wave, lane);
    store_acc(out, C, ld, crow, ccol);
    if (stamp) STAMP(10);
    if (wtr) wtr[1] = wall_clock64();
}

// Task tables (see potrf_step_kernel): one vector of tasks per launch, cached on the device per (nbk, inverse).
struct TaskTable {
    int4 *dev = nullptr;
    std::vector<int> offset, count, nhead, npanel;
    std::vector<double> tile_ops;   // 64^3 multiply-add units per launch and matrix (for the profiler)
};

#ifndef PANEL_LEAD
#define PANEL_LEAD 1024   // bulk workgroups dispatched before the (waiting) panel workgroups of a launch
#endif

static int step_kernel_wgs_per_cu();
int get_tasks(dgpamd_ctx *ctx, int nbk, bool inv, TaskTable *&out) {
    (void)step_kernel_wgs_per_cu();   // (occupancy query: on first use, outside a graph capture as the upload below)
    static std::map<std::pair<dgpamd_ctx *, std::pair<int, int>>, TaskTable> cache;   // contexts are few and long-lived
    TaskTable &tt = cache[{ctx, {nbk, inv ? 1 : 0}}];
    if (!tt.dev) {
        std::vector<std::vector<Task4>> L;
        build_tasks(nbk, inv, L, tt.tile_ops);
        std::vector<Task4> flat;
        for (auto &v : L) {
            tt.offset.push_back((int)flat.size());
            tt.count.push_back((int)v.size());
            int nh = 0, np_ = 0;
            for (auto &t4 : v) {
                const int post = task_post(t4.x);
                nh += (post == T_CHAIN || post == T_TDIAG);
                np_ += (post == T_SOLVE);
            }
            tt.nhead.push_back(nh);
            tt.npanel.push_back(np_);
            flat.insert(flat.end(), v.begin(), v.end());
        }
        HIP_TRY(ctx, hipMalloc((void **)&tt.dev, flat.size() * sizeof(int4)));
        HIP_TRY(ctx, hipMemcpy(tt.dev, flat.data(), flat.size() * sizeof(int4), hipMemcpyHostToDevice));
    }
    out = &tt;
    return DGPAMD_OK;
}

// workgroups of potrf_step_kernel that one CU holds (registers / LDS): decides how many placeholder rows guard a chain
static int step_kernel_wgs_per_cu() {
    static int n = 0;
    if (!n) {
        int q = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, potrf_step_kernel, 256, 0) != hipSuccess || q < 1) q = 2;
        n = q > 4 ? 4 : q;
    }
    return n;
}

int potrf_launches(dgpamd_ctx *ctx, int64_t n, double *A, double *T, double *S, int64_t stride_a, int batch,
                   double *logdet, int32_t *info, double *ws, int32_t *flags, const TaskTable *tt) {
    const int64_t Np = padded_dim(n);
    const int nbk = (int)(Np / 64);
    const double tile_flops = 2.0 * 64.0 * 64.0 * 64.0;
    HIP_TRY(ctx, hipMemsetAsync(flags, 0, 2 * DGPAMD_MAXB * sizeof(int32_t), ctx->stream));
    StepArgs st;
    st.buf[BUF_A] = A; st.buf[BUF_T] = T; st.buf[BUF_S] = S;
    st.ws = ws; st.ld = Np; st.stride_a = stride_a; st.stride_ws = (int64_t)nbk * 4096; st.n = n; st.nbk = nbk;
    st.logdet = logdet; st.info = info; st.flags = flags; st.batch = batch; st.trace = ctx->trace;
    for (size_t k = 0; k < tt->count.size(); ++k) {
        if (tt->count[k] == 0) continue;
        st.k = (int)k;
        st.tasks = tt->dev + tt->offset[k];
        st.nhead = tt->nhead[k];
        st.npanel = tt->npanel[k];
        {
            const int nbulk = tt->count[k] - st.nhead - st.npanel, lead = (PANEL_LEAD + batch - 1) / batch;
            st.lead = lead < nbulk ? lead : nbulk;
        }
        const int64_t nwg = (int64_t)batch * tt->count[k];
        st.guard = (k < (size_t)nbk && nwg > ctx->num_cu) ? ctx->num_cu : 0;   // (tail launches: no chain; small ones: no neighbours)
        st.nph = step_kernel_wgs_per_cu() - 1;
        int64_t grid = nwg;
        if (st.guard)   // smallest grid that holds nwg tasks beside the placeholders of the rows it reaches
            for (int m = 1; m <= st.nph && grid > (int64_t)m * st.guard; ++m) grid += batch;
        PROF_BEGIN(ctx, PROF_SYRK, (double)batch * tt->tile_ops[k] * tile_flops);
        hipLaunchKernelGGL(potrf_step_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, st);
        PROF_END(ctx, PROF_SYRK);
    }
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
