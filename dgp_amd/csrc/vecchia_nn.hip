// Vecchia neighbour search (reference dgpsi/vecchia.py:20-40,100-108): exact brute force on device, in
// (distance, index) order -> deterministic.
#include "common.hpp"
#include "wave.hpp"

#include <math.h>

// ---------------------------------------------------------------------------
// a17  neighbour search
// ---------------------------------------------------------------------------
// The selection passes of the two kernels below.  Pass p selects the p-th smallest (dist, index) pair (pair_less) of the
// `count` candidates into sel[p]; cand(j, d, i) yields candidate j's pair -- recomputed, from the short LDS list or from
// the stored row.  rd / ri: the four waves' minima.
template <class CAND>
__device__ __forceinline__ void nn_select_passes(int k, int64_t count, double *rd, int64_t *ri, int64_t *sel, CAND cand) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double pd = -1.0;
    int64_t pi = -1;
    for (int pass = 0; pass < k; ++pass) {
        double bd = INFINITY;
        int64_t bidx = INT64_MAX;
        for (int64_t j = tid; j < count; j += 256) {
            double s;
            int64_t i;
            cand(j, s, i);
            if (pair_less(pd, pi, s, i) && pair_less(s, i, bd, bidx)) {
                bd = s;
                bidx = i;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            double od = __shfl_down(bd, off, 64);
            int64_t oi = __shfl_down(bidx, off, 64);
            if (pair_less(od, oi, bd, bidx)) {
                bd = od;
                bidx = oi;
            }
        }
        if (lane == 0) {
            rd[wave] = bd;
            ri[wave] = bidx;
        }
        __syncthreads();
        bd = rd[0];
        bidx = ri[0];
        for (int w = 1; w < 4; ++w)
            if (pair_less(rd[w], ri[w], bd, bidx)) {
                bd = rd[w];
                bidx = ri[w];
            }
        pd = bd;
        pi = bidx;
        if (tid == 0) sel[pass] = bidx;
        __syncthreads();
    }
}

// (one thread) the k selected indices to the query's row of the output, -1 padded
__device__ __forceinline__ void nn_write_out(int64_t *sel, int k, int m_out, int ordered, int64_t *out) {
    if (ordered) {   // vecchia.py:108  np.fliplr(np.sort(NNarray)): index-descending, -1 padded
        for (int a = 1; a < k; ++a) {
            int64_t v = sel[a];
            int b = a - 1;
            while (b >= 0 && sel[b] < v) {
                sel[b + 1] = sel[b];
                --b;
            }
            sel[b + 1] = v;
        }
    }
    for (int a = 0; a < m_out; ++a) out[a] = a < k ? sel[a] : -1;
}

// One 256-thread workgroup per query, every distance recomputed in every pass.
__global__ __launch_bounds__(256) void nn_select_kernel(int64_t nq, int64_t nx, int D, const double *q, const double *x,
                                                        int m_out, int ordered, int64_t *out) {
    extern __shared__ double lds[];
    double *qs = lds;                                  // [D]
    double *rd = lds + D;                              // [4] wave minima (dist)
    int64_t *ri = reinterpret_cast<int64_t *>(rd + 4); // [4] wave minima (index)
    int64_t *sel = ri + 4;                             // [m_out] selected indices
    const int tid = threadIdx.x;
    const int64_t iq = blockIdx.x;
    const int64_t ncand = ordered ? iq + 1 : nx;       // ordered: only points with index <= own
    const int k = (int)(ncand < m_out ? ncand : m_out);
    for (int d = tid; d < D; d += 256) qs[d] = q[iq * D + d];
    __syncthreads();
    nn_select_passes(k, ncand, rd, ri, sel, [&](int64_t j, double &s, int64_t &i) {
        s = 0.0;
        for (int d = 0; d < D; ++d) {
            double df = x[j * D + d] - qs[d];
            s = fma(df, df, s);
        }
        i = j;
    });
    if (tid == 0) nn_write_out(sel, k, m_out, ordered, out + iq * m_out);
}

// Large candidate sets: the m_out selection passes above recompute every distance every pass.  Here a workgroup writes
// the distances of its query ONCE (global scratch row), narrows them with a 1024-bin histogram (zooming into the bin
// that holds the k-th smallest until at most NN_CMAX candidates are left), gathers those into LDS and runs the same
// (distance, index)-ordered selection passes on that short list -- identical output, ~m_out times less arithmetic.
// Workgroups are persistent over the queries (grid-stride), one scratch row each.
#define NN_NB 1024
#define NN_CMAX 2048
__global__ __launch_bounds__(256) void nn_select_big_kernel(int64_t nq, int64_t nx, int D, const double *q, const double *x,
                                                            int m_out, int ordered, int64_t *out, double *scratch) {
    extern __shared__ double lds[];
    double *qs = lds;                                   // [D]
    double *rd = qs + D;                                // [8] wave partials
    double *cd = rd + 8;                                // [NN_CMAX] candidate distances
    int64_t *ci = reinterpret_cast<int64_t *>(cd + NN_CMAX);   // [NN_CMAX] candidate indices
    int64_t *ri = ci + NN_CMAX;                         // [4]
    int64_t *sel = ri + 4;                              // [m_out]
    int *hist = reinterpret_cast<int *>(sel + m_out);   // [NN_NB]
    int *part = hist + NN_NB;                           // [256]
    int *ctrl = part + 256;                             // [4]: bin*, count below bin*, candidate counter
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double *dist = scratch + (int64_t)blockIdx.x * nx;
    for (int64_t iq = blockIdx.x; iq < nq; iq += gridDim.x) {
        const int64_t ncand = ordered ? iq + 1 : nx;
        const int k = (int)(ncand < m_out ? ncand : m_out);
        __syncthreads();
        for (int d = tid; d < D; d += 256) qs[d] = q[iq * D + d];
        __syncthreads();
        // ---- distances, once
        double lo = INFINITY, hi = -INFINITY;
        for (int64_t j = tid; j < ncand; j += 256) {
            double s = 0.0;
            for (int d = 0; d < D; ++d) {
                double df = x[j * D + d] - qs[d];
                s = fma(df, df, s);
            }
            dist[j] = s;
            lo = fmin(lo, s);
            hi = fmax(hi, s);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = fmin(lo, __shfl_down(lo, off, 64));
            hi = fmax(hi, __shfl_down(hi, off, 64));
        }
        if (lane == 0) {
            rd[wave] = lo;
            rd[4 + wave] = hi;
        }
        __syncthreads();
        lo = fmin(fmin(rd[0], rd[1]), fmin(rd[2], rd[3]));
        hi = fmax(fmax(rd[4], rd[5]), fmax(rd[6], rd[7]));
        // ---- zoom: histogram of the values <= hi, find the bin of the k-th smallest
        int ncollect = 0;
        bool listed = false;
        for (int zoom = 0; zoom < 6; ++zoom) {
            const double scale = hi > lo ? (double)NN_NB / (hi - lo) : 0.0;
            __syncthreads();
            for (int b = tid; b < NN_NB; b += 256) hist[b] = 0;
            __syncthreads();
            for (int64_t j = tid; j < ncand; j += 256) {
                const double s = dist[j];
                if (s <= hi) {
                    int b = (int)((s - lo) * scale);
                    atomicAdd(&hist[b < NN_NB ? b : NN_NB - 1], 1);
                }
            }
            __syncthreads();
            part[tid] = hist[4 * tid] + hist[4 * tid + 1] + hist[4 * tid + 2] + hist[4 * tid + 3];
            __syncthreads();
            if (tid == 0) {
                int cum = 0, c = 0;
                while (c < 255 && cum + part[c] < k) cum += part[c++];
                int b = 4 * c;
                while (b < 4 * c + 3 && cum + hist[b] < k) cum += hist[b++];
                ctrl[0] = b;
                ctrl[1] = cum + hist[b];   // everything in the bins <= b
                ctrl[2] = 0;
            }
            __syncthreads();
            const int bstar = ctrl[0];
            ncollect = ctrl[1];
            if (ncollect <= NN_CMAX) {
                for (int64_t j = tid; j < ncand; j += 256) {
                    const double s = dist[j];
                    if (s <= hi) {
                        int b = (int)((s - lo) * scale);
                        b = b < NN_NB ? b : NN_NB - 1;
                        if (b <= bstar) {
                            const int pos = atomicAdd(&ctrl[2], 1);
                            cd[pos] = s;
                            ci[pos] = j;
                        }
                    }
                }
                listed = true;
                break;
            }
            // too many: keep only the bins <= b* and spread them over the histogram again.  The new upper end is the
            // largest VALUE kept (an exact, monotone filter: s <= nhi <=> bin(s) <= b*), not a recomputed bin edge.
            double nhi = -INFINITY;
            for (int64_t j = tid; j < ncand; j += 256) {
                const double s = dist[j];
                if (s <= hi) {
                    int b = (int)((s - lo) * scale);
                    b = b < NN_NB ? b : NN_NB - 1;
                    if (b <= bstar) nhi = fmax(nhi, s);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) nhi = fmax(nhi, __shfl_down(nhi, off, 64));
            __syncthreads();
            if (lane == 0) rd[wave] = nhi;
            __syncthreads();
            nhi = fmax(fmax(rd[0], rd[1]), fmax(rd[2], rd[3]));
            if (!(nhi < hi) && bstar == NN_NB - 1) break;   // nothing was cut off
            if (!(nhi > lo)) break;                          // all remaining values equal: ties, stored-distance passes
            hi = nhi;
        }
        __syncthreads();
        // ---- selection passes in (distance, index) order, over the short list or (ties) over the stored distances
        if (listed)
            nn_select_passes(k, ncollect, rd, ri, sel, [&](int64_t c, double &s, int64_t &i) { s = cd[c]; i = ci[c]; });
        else
            nn_select_passes(k, ncand, rd, ri, sel, [&](int64_t j, double &s, int64_t &i) { s = dist[j]; i = j; });
        if (tid == 0) nn_write_out(sel, k, m_out, ordered, out + iq * m_out);
    }
}

// ---------------------------------------------------------------------------
// Large candidate sets, few dimensions, at most 64 neighbours: a streaming top-k.  The store-once kernel above reads
// the candidate array once per QUERY (n^2/2 x 64 B = 80 GB of L2 traffic at n = 50 000: it runs at the L2's bandwidth)
// and then passes over n stored distances several times more.  Here a wave takes 64 queries, one per lane, and one chunk
// of the candidate range: 64 candidates at a time are staged in LDS and every lane reads them with wave-uniform
// (broadcast) addresses -- each candidate byte is loaded once per 64 queries.  A lane keeps its K best (distance, index)
// pairs SORTED IN REGISTERS; a candidate that beats the lane's K-th best bubbles in (K compare-and-swap steps, executed
// only when some lane of the wave has one: a quarter of the candidates at n = 50 000, K = 26).  The partial lists of the
// chunks go to global scratch and a second kernel merges them the same way and writes the output in the order the
// selection passes above produce.  Distances use the same fma chain, the order is the same (distance, index) order:
// identical neighbour arrays.
// ---------------------------------------------------------------------------
#include <limits.h>

template <int K>
__device__ __forceinline__ void topk_insert(double (&ld)[K], int (&li)[K], double cd, int ci) {
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const bool sw = cd < ld[t] || (cd == ld[t] && ci < li[t]);
        const double od = ld[t];
        const int oi = li[t];
        ld[t] = sw ? cd : od;
        li[t] = sw ? ci : oi;
        cd = sw ? od : cd;
        ci = sw ? oi : ci;
    }
}

#define NN_PEND 16   // accepted candidates a lane may hold back before the wave merges them into the sorted lists (8: 15 % slower in the query form -- the
                     // passes of a flush are as many as the fullest lane holds, mostly empty for the others; 32: the ordered search loses occupancy to the 24 KB of notes)

template <int DMAX, int K>
__global__ __launch_bounds__(64) void nn_scan_kernel(int64_t nq, int64_t nx, int D, const double *__restrict__ q,
                                                     const double *__restrict__ x, int ordered, int64_t chunk, int nchunk,
                                                     double *__restrict__ sd, int *__restrict__ si) {
    __shared__ __attribute__((aligned(16))) double tile[64 * DMAX];
    __shared__ double pend_d[NN_PEND * 64];
    __shared__ int pend_i[NN_PEND * 64];
    const int lane = threadIdx.x;
    const int64_t nblk = (nq + 63) / 64;
    const int64_t qb = ordered ? nblk - 1 - blockIdx.x : blockIdx.x;   // (ordered: the long scans first)
    const int64_t iq = qb * 64 + lane;
    const bool qlive = iq < nq;
    const int64_t nscan = ordered ? (qb * 64 + 64 < nx ? qb * 64 + 64 : nx) : nx;
    const int64_t lo = (int64_t)blockIdx.y * chunk;
    if (lo >= nscan) return;
    const int64_t hi = lo + chunk < nscan ? lo + chunk : nscan;
    const int64_t mine = ordered ? iq + 1 : nx;   // candidates j < mine
    double qv[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) qv[d] = (qlive && d < D) ? q[iq * D + d] : 0.0;
    double ld[K];
    int li[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        ld[t] = INFINITY;
        li[t] = INT_MAX;
    }
    // A candidate below the lane's K-th best is only NOTED (LDS); when some lane has noted NN_PEND of them the whole wave
    // bubbles its notes into the sorted lists: one pass of K compare-and-swap steps then serves up to 64 insertions
    // instead of one.  Until then the threshold is the old K-th best -- a few notes more than necessary, the same result.
    double tau = INFINITY;
    int cnt = 0;
    auto flush = [&]() {
        // (a LOOP over the passes: unrolled, the NN_PEND copies of the K-step insertion are 40 KB of code per call site, more
        //  than the instruction cache holds, and the waves -- each at another point of it -- ran at the speed of its misses)
#pragma unroll 1
        for (int p = 0; p < NN_PEND; ++p) {
            const bool have = p < cnt;
            if (!__any(have)) break;
            topk_insert<K>(ld, li, have ? pend_d[p * 64 + lane] : INFINITY, have ? pend_i[p * 64 + lane] : INT_MAX);
        }
        cnt = 0;
        tau = ld[K - 1];
    };
    for (int64_t base = lo; base < hi; base += 64) {
        const int64_t jc = base + lane;
        __syncthreads();
#pragma unroll
        for (int d = 0; d < DMAX; ++d) tile[lane * DMAX + d] = (jc < hi && d < D) ? x[jc * D + d] : 0.0;
        __syncthreads();
        const int cnt_c = (int)(hi - base < 64 ? hi - base : 64);
        for (int c = 0; c < cnt_c; ++c) {
            double s = 0.0;
#pragma unroll
            for (int d = 0; d < DMAX; ++d) {   // (dimensions past D: 0 - 0, fma(0, 0, s) = s)
                const double df = tile[c * DMAX + d] - qv[d];
                s = fma(df, df, s);
            }
            const int64_t j = base + c;
            const bool take = qlive && j < mine && s < tau;   // (equal distance: the earlier index stays)
            if (__any(take)) {
                if (take) {
                    pend_d[cnt * 64 + lane] = s;
                    pend_i[cnt * 64 + lane] = (int)j;
                    ++cnt;
                }
                if (__any(cnt == NN_PEND)) flush();
            }
        }
    }
    flush();
    const int64_t item = qb * nchunk + blockIdx.y;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        sd[(item * K + t) * 64 + lane] = ld[t];
        si[(item * K + t) * 64 + lane] = li[t];
    }
}

template <int K>
__global__ __launch_bounds__(64) void nn_merge_kernel(int64_t nq, int64_t nx, int m_out, int ordered, int64_t chunk, int nchunk,
                                                      const double *__restrict__ sd, const int *__restrict__ si,
                                                      int64_t *__restrict__ out) {
    const int lane = threadIdx.x;
    const int64_t qb = blockIdx.x, iq = qb * 64 + lane;
    const int64_t nscan = ordered ? (qb * 64 + 64 < nx ? qb * 64 + 64 : nx) : nx;
    const int nch = (int)((nscan + chunk - 1) / chunk);
    double ld[K];
    int li[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        ld[t] = sd[((qb * nchunk) * K + t) * 64 + lane];
        li[t] = si[((qb * nchunk) * K + t) * 64 + lane];
    }
    for (int c = 1; c < nch; ++c) {
        const int64_t item = qb * nchunk + c;
#pragma unroll 1   // (unrolled this was K copies of the K-step insertion: 137 KB of code at K = 51)
        for (int t = 0; t < K; ++t) {
            const double cd = sd[(item * K + t) * 64 + lane];
            const int ci = si[(item * K + t) * 64 + lane];
            if (__any(cd < ld[K - 1] || (cd == ld[K - 1] && ci < li[K - 1]))) topk_insert<K>(ld, li, cd, ci);
        }
    }
    if (iq >= nq) return;
    const int64_t mine = ordered ? iq + 1 : nx;
    const int kk = (int)(mine < m_out ? mine : m_out);   // valid neighbours: the first kk of the sorted list
    if (!ordered) {
#pragma unroll
        for (int t = 0; t < K; ++t)
            if (t < m_out) out[iq * m_out + t] = t < kk ? li[t] : -1;
        return;
    }
    // vecchia.py:108  np.fliplr(np.sort(NNarray)): index-descending, -1 padded
    for (int t = kk; t < m_out; ++t) out[iq * m_out + t] = -1;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        if (t < kk) {
            int pos = 0;
#pragma unroll
            for (int u = 0; u < K; ++u) pos += (u < kk && li[u] > li[t]);
            out[iq * m_out + pos] = li[t];
        }
    }
}

template <int DMAX, int K>
static int launch_nn_stream(dgpamd_ctx *ctx, int64_t nq, int64_t nx, int D, const double *q, const double *x, int m_out, int ordered,
                            int64_t *out) {
    const int64_t nblk = (nq + 63) / 64;
    // chunks of the candidate range: enough (block, chunk) items to fill the chip, at most 8192 candidates each
    int64_t chunk = (nx * nblk / 4096 + 63) / 64 * 64;
    chunk = chunk < 1024 ? 1024 : (chunk > 8192 ? 8192 : chunk);
    // measured (n = 50 000, d = 8): every chunk starts with empty lists, so the query form -- few blocks of queries, each scanning
    // everything -- wants long chunks (10 000 queries: 9.8 ms with 1920-candidate chunks, 4.9 ms with 8192); the ordered search
    // has blocks enough and only gains from 16384 at the largest sizes (4.1 -> 3.7 ms at n = 50 000)
    if (!ordered)
        chunk = nq < 15000 ? 8192 : (nq < 40000 ? 16384 : 25024);
    else if (nx >= 45000)
        chunk = 16384;
    const int nchunk = (int)((nx + chunk - 1) / chunk);
    const size_t items = (size_t)nblk * nchunk;
    void *both = nullptr;
    int rc = ctx_scratch(ctx, 1, items * K * 64 * (sizeof(double) + sizeof(int)), &both);
    if (rc) return rc;
    double *sd = reinterpret_cast<double *>(both);
    int *si = reinterpret_cast<int *>(sd + items * K * 64);
    hipLaunchKernelGGL((nn_scan_kernel<DMAX, K>), dim3((unsigned)nblk, (unsigned)nchunk), dim3(64), 0, ctx->stream, nq, nx, D, q, x,
                       ordered, chunk, nchunk, sd, si);
    hipLaunchKernelGGL((nn_merge_kernel<K>), dim3((unsigned)nblk), dim3(64), 0, ctx->stream, nq, nx, m_out, ordered, chunk, nchunk,
                       (const double *)sd, (const int *)si, out);
    return DGPAMD_OK;
}

// ---------------------------------------------------------------------------
// Round 5, the QUERY form (vecchia.py:20-40) at prediction sizes -- 1e5 queries against 5e4 points, 50 neighbours: filter, then select.
// The streaming kernel above keeps K = 51 sorted pairs per lane in registers: 256 VGPRs, ONE wave per SIMD, so every LDS read
// and every dependent issue of its distance loop was exposed (one instruction per ~11 cycles; 43 ms at D = 16, a third of what its
// own instruction count needs).  The top-k state does not have to ride along the scan:
//   (A) nn_tau_kernel: per query the r-th smallest distance to a strided sample of S candidates (a small sorted list: r <= 32) -- an
//       upper bound tau of its K-th nearest distance unless fewer than K of ALL candidates lie at or below it (r is chosen so that
//       this has probability ~1e-8 per query, and it is CHECKED);
//   (B) nn_collect_kernel: the scan itself -- 256 queries per workgroup share the staged candidates, a lane holds its query and tau
//       (~60 VGPRs: five waves per SIMD) and notes every candidate with distance <= tau, through LDS, in a region of global memory of
//       its own (per query and candidate chunk: no atomics);
//   (C) nn_pick_kernel: per query the K nearest of its few hundred notes, by the same (distance, index) insertion as above.  A query
//       whose notes are fewer than K, or overflowed their region, is scanned exactly by its lane (the rare slow path).
// The distances are the same fma chains, the order the same (distance, index) order: identical neighbour arrays (tests).
// ---------------------------------------------------------------------------
#define NNF_R 32        // sample list length (r <= NNF_R)
#define NNF_PEND 8      // notes a lane holds in LDS before the wave writes them out

template <int DMAX>
__global__ __launch_bounds__(64) void nn_tau_kernel(int64_t nq, int64_t nx, int D, const double *__restrict__ q, const double *__restrict__ x,
                                                    int64_t S, int64_t stride, int r, double *__restrict__ tau) {
    __shared__ __attribute__((aligned(16))) double tile[64 * DMAX];
    const int lane = threadIdx.x;
    const int64_t iq = (int64_t)blockIdx.x * 64 + lane;
    const bool qlive = iq < nq;
    double qv[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) qv[d] = (qlive && d < D) ? q[iq * D + d] : 0.0;
    double ld[NNF_R];
    int li[NNF_R];
#pragma unroll
    for (int t = 0; t < NNF_R; ++t) {
        ld[t] = INFINITY;
        li[t] = INT_MAX;
    }
    for (int64_t base = 0; base < S; base += 64) {
        const int64_t js = (base + lane) * stride;   // the sample: every stride-th candidate
        __syncthreads();
#pragma unroll
        for (int d = 0; d < DMAX; ++d) tile[lane * DMAX + d] = (base + lane < S && js < nx && d < D) ? x[js * D + d] : 0.0;
        __syncthreads();
        const int cnt_c = (int)(S - base < 64 ? S - base : 64);
        for (int c = 0; c < cnt_c; ++c) {
            double sacc = 0.0;
#pragma unroll
            for (int d = 0; d < DMAX; ++d) {
                const double df = tile[c * DMAX + d] - qv[d];
                sacc = fma(df, df, sacc);
            }
            if (__any(sacc < ld[NNF_R - 1])) topk_insert<NNF_R>(ld, li, sacc, (int)(base + c));
        }
    }
    double t = ld[0];
#pragma unroll
    for (int u = 1; u < NNF_R; ++u) t = (u < r) ? ld[u] : t;   // the r-th smallest
    if (qlive) tau[iq] = t;
}

// grid (query blocks of 256, candidate chunks); notes of query iq in chunk ch: nd / ni [(iq * nchunk + ch) * capc ...], count in ncnt
template <int DMAX>
__global__ __launch_bounds__(256) void nn_collect_kernel(int64_t nq, int64_t nx, int D, const double *__restrict__ q, const double *__restrict__ x,
                                                         const double *__restrict__ tau, int64_t chunk, int nchunk, int capc,
                                                         double *__restrict__ nd, int *__restrict__ ni, int *__restrict__ ncnt) {
    __shared__ __attribute__((aligned(16))) double tile[64 * DMAX];
    __shared__ double pend_d[4][NNF_PEND * 64];
    __shared__ int pend_i[4][NNF_PEND * 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t iq = (int64_t)blockIdx.x * 256 + tid;
    const bool qlive = iq < nq;
    const int64_t lo = (int64_t)blockIdx.y * chunk, hi = lo + chunk < nx ? lo + chunk : nx;
    double qv[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) qv[d] = (qlive && d < D) ? q[iq * D + d] : 0.0;
    const double tq = qlive ? tau[iq] : -1.0;
    double *mynd = nd + (iq * nchunk + blockIdx.y) * (int64_t)capc;
    int *myni = ni + (iq * nchunk + blockIdx.y) * (int64_t)capc;
    int cnt = 0, tot = 0;
    auto flush = [&]() {
        for (int p = 0; p < cnt; ++p)
            if (tot + p < capc) {
                mynd[tot + p] = pend_d[wave][p * 64 + lane];
                myni[tot + p] = pend_i[wave][p * 64 + lane];
            }
        tot += cnt;   // (beyond capc: counted, not stored -- the pick kernel sees the overflow)
        cnt = 0;
    };
    for (int64_t base = lo; base < hi; base += 64) {
        __syncthreads();
        {   // 64 candidates x DMAX doubles, staged by all 256 threads
            const int c = tid >> 2, d0 = (tid & 3) * (DMAX / 4);
            const int64_t jc = base + c;
#pragma unroll
            for (int d = 0; d < DMAX / 4; ++d) tile[c * DMAX + d0 + d] = (jc < hi && d0 + d < D) ? x[jc * D + d0 + d] : 0.0;
        }
        __syncthreads();
        const int cnt_c = (int)(hi - base < 64 ? hi - base : 64);
        for (int c = 0; c < cnt_c; c += 2) {   // two candidates per pass: independent chains
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int d = 0; d < DMAX; ++d) {
                const double d0 = tile[c * DMAX + d] - qv[d], d1 = tile[(c + 1) * DMAX + d] - qv[d];   // (c + 1 == cnt_c: a zero-padded row, never taken)
                s0 = fma(d0, d0, s0);
                s1 = fma(d1, d1, s1);
            }
            const bool t0 = s0 <= tq, t1 = c + 1 < cnt_c && s1 <= tq;
            if (__any(t0 || t1)) {
                if (t0) {
                    pend_d[wave][cnt * 64 + lane] = s0;
                    pend_i[wave][cnt * 64 + lane] = (int)(base + c);
                    ++cnt;
                }
                if (__any(cnt == NNF_PEND)) flush();
                if (t1) {
                    pend_d[wave][cnt * 64 + lane] = s1;
                    pend_i[wave][cnt * 64 + lane] = (int)(base + c + 1);
                    ++cnt;
                }
                if (__any(cnt == NNF_PEND)) flush();
            }
        }
    }
    flush();
    if (qlive) ncnt[iq * nchunk + blockIdx.y] = tot;
}

template <int DMAX, int K>
__global__ __launch_bounds__(64) void nn_pick_kernel(int64_t nq, int64_t nx, int D, const double *__restrict__ q, const double *__restrict__ x,
                                                     int nchunk, int capc, const double *__restrict__ nd, const int *__restrict__ ni,
                                                     const int *__restrict__ ncnt, int m_out, int64_t *__restrict__ out, int *__restrict__ slow) {
    const int lane = threadIdx.x;
    const int64_t iq = (int64_t)blockIdx.x * 64 + lane;
    const bool qlive = iq < nq;
    double ld[K];
    int li[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        ld[t] = INFINITY;
        li[t] = INT_MAX;
    }
    int total = 0;
    bool over = false;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int c0 = qlive ? ncnt[iq * nchunk + ch] : 0;
        over |= c0 > capc;
        const int cn = c0 < capc ? c0 : capc;
        total += cn;
        const double *mynd = nd + (iq * nchunk + ch) * (int64_t)capc;
        const int *myni = ni + (iq * nchunk + ch) * (int64_t)capc;
        int cmax = cn;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(cmax, off, 64);
            cmax = o > cmax ? o : cmax;
        }
#pragma unroll 1
        for (int p = 0; p < cmax; ++p) {
            const bool have = p < cn;
            const double cd = have ? mynd[p] : INFINITY;
            const int ci = have ? myni[p] : INT_MAX;
            if (__any(cd < ld[K - 1] || (cd == ld[K - 1] && ci < li[K - 1]))) topk_insert<K>(ld, li, cd, ci);
        }
    }
    // the rare slow path: too few notes (the sampled bound was below the K-th nearest distance) or an overflowed region -- the lane
    // scans every candidate itself (same chain, same order)
    const int need = (int)(nx < m_out ? nx : m_out);
    const bool bad = qlive && (over || total < need);
    if (__any(bad)) {
        if (bad) {
#pragma unroll
            for (int t = 0; t < K; ++t) {
                ld[t] = INFINITY;
                li[t] = INT_MAX;
            }
            atomicAdd(slow, 1);
        }
        double qv[DMAX];
#pragma unroll
        for (int d = 0; d < DMAX; ++d) qv[d] = (qlive && d < D) ? q[iq * D + d] : 0.0;
#pragma unroll 1
        for (int64_t j = 0; j < nx; ++j) {
            double sacc = 0.0;
#pragma unroll
            for (int d = 0; d < DMAX; ++d) {
                const double df = (d < D ? x[j * D + d] : 0.0) - qv[d];
                sacc = fma(df, df, sacc);
            }
            const bool take = bad && sacc < ld[K - 1];   // (equal distance: the earlier index stays)
            if (__any(take)) topk_insert<K>(ld, li, take ? sacc : INFINITY, take ? (int)j : INT_MAX);
        }
    }
    if (!qlive) return;
    const int kk = (int)(nx < m_out ? nx : m_out);
#pragma unroll
    for (int t = 0; t < K; ++t)
        if (t < m_out) out[iq * m_out + t] = t < kk ? li[t] : -1;
}

// The filter pipeline's plan for (nq, nx, K): sample size, rank, chunking, region capacity; false when the shape does not suit it
struct NnfPlan {
    int64_t S, stride, chunk;
    int r, nchunk, capc;
};
static bool nnf_plan(int64_t nq, int64_t nx, int K, NnfPlan &p) {
    if (nq < 30000 || nx < 20000 || nx >= INT_MAX) return false;   // (measured: below ~25 000 queries the streaming kernel is as fast or faster)
    p.S = nx / 16 < 2048 ? 2048 : (nx / 16 > 8192 ? 8192 : nx / 16);
    p.stride = nx / p.S;
    const double lam = (double)K * (double)p.S / (double)nx;             // sample points expected among the K nearest
    const double rr = lam + 6.0 * sqrt(lam) + 6.0;                         // P(Poisson(lam) >= r) ~ 1e-8: the bound then holds K candidates
    if (rr > NNF_R) return false;
    p.r = (int)ceil(rr);
    const double en = (double)p.r * (double)nx / (double)p.S;            // candidates expected at or below tau, +- en / sqrt(r)
    // two chunks of candidates (the collect kernel is fast enough for 392 x 2 workgroups to fill the chip at 1e5 queries); more for few queries
    p.nchunk = nq >= 60000 ? 2 : (nq >= 25000 ? 4 : 8);
    p.chunk = ((nx + p.nchunk - 1) / p.nchunk + 63) / 64 * 64;
    p.nchunk = (int)((nx + p.chunk - 1) / p.chunk);
    const double per = en / p.nchunk * (1.0 + 5.0 / sqrt((double)p.r)) + 64.0;   // a region: its share at + 5 sigma of the rank's spread
    p.capc = ((int)per + 63) / 64 * 64;
    return (double)nq * p.nchunk * p.capc * 12.0 <= 1.5e9;                 // (scratch: <= 1.5 GB, else the streaming kernel)
}

template <int DMAX, int K>
static int launch_nn_filter(dgpamd_ctx *ctx, int64_t nq, int64_t nx, int D, const double *q, const double *x, int m_out, int64_t *out,
                            const NnfPlan &p) {
    const size_t nreg = (size_t)nq * p.nchunk;
    const size_t bytes = nreg * p.capc * 12 + nreg * 4 + (size_t)nq * 8 + 64;
    void *both = nullptr;
    int rc = ctx_scratch(ctx, 1, bytes, &both);
    if (rc) return rc;
    double *nd = reinterpret_cast<double *>(both);
    double *tau = nd + nreg * p.capc;
    int *ni = reinterpret_cast<int *>(tau + nq);
    int *ncnt = ni + nreg * p.capc;
    int *slow = ncnt + nreg;
    HIP_TRY(ctx, hipMemsetAsync(slow, 0, 4, ctx->stream));
    hipLaunchKernelGGL((nn_tau_kernel<DMAX>), dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, ctx->stream, nq, nx, D, q, x, p.S, p.stride, p.r, tau);
    hipLaunchKernelGGL((nn_collect_kernel<DMAX>), dim3((unsigned)((nq + 255) / 256), (unsigned)p.nchunk), dim3(256), 0, ctx->stream, nq, nx, D, q, x,
                       (const double *)tau, p.chunk, p.nchunk, p.capc, nd, ni, ncnt);
    hipLaunchKernelGGL((nn_pick_kernel<DMAX, K>), dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, ctx->stream, nq, nx, D, q, x, p.nchunk, p.capc,
                       (const double *)nd, (const int *)ni, (const int *)ncnt, m_out, out, slow);
    return DGPAMD_OK;
}

template <int DMAX>
static int launch_nn_stream_k(dgpamd_ctx *ctx, int64_t nq, int64_t nx, int D, const double *q, const double *x, int m_out,
                              int ordered, int64_t *out) {
    // the query form at prediction sizes: filter, then select (DGPAMD_NN_FILTER=0: the streaming kernel, for comparisons)
    const bool filter_on = ctx->tune.nn_filter != 0;
    NnfPlan plan;
    if (!ordered && filter_on && m_out > 26 && nnf_plan(nq, nx, m_out, plan)) {
        if (m_out <= 32) return launch_nn_filter<DMAX, 32>(ctx, nq, nx, D, q, x, m_out, out, plan);
        if (m_out <= 51) return launch_nn_filter<DMAX, 51>(ctx, nq, nx, D, q, x, m_out, out, plan);
        return launch_nn_filter<DMAX, 64>(ctx, nq, nx, D, q, x, m_out, out, plan);
    }
    if (m_out <= 16) return launch_nn_stream<DMAX, 16>(ctx, nq, nx, D, q, x, m_out, ordered, out);
    if (m_out <= 26) return launch_nn_stream<DMAX, 26>(ctx, nq, nx, D, q, x, m_out, ordered, out);
    if (m_out <= 32) return launch_nn_stream<DMAX, 32>(ctx, nq, nx, D, q, x, m_out, ordered, out);
    if (m_out <= 51) return launch_nn_stream<DMAX, 51>(ctx, nq, nx, D, q, x, m_out, ordered, out);
    return launch_nn_stream<DMAX, 64>(ctx, nq, nx, D, q, x, m_out, ordered, out);
}

#define NN_BIG_MIN 4096   // candidate sets from this size on take the store-once path
static int launch_nn(dgpamd_ctx *ctx, int64_t nq, int64_t nx, int D, const double *q, const double *x, int m_out, int ordered,
                     int64_t *out) {
    if (nx < NN_BIG_MIN) {
        size_t shm = (D + 4) * sizeof(double) + (4 + (size_t)m_out) * sizeof(int64_t);
        hipLaunchKernelGGL(nn_select_kernel, dim3((unsigned)nq), dim3(256), shm, ctx->stream, nq, nx, D, q, x, m_out, ordered, out);
        return DGPAMD_OK;
    }
    // measured crossovers (tools/gpu_nn_bench.py): the streaming kernels win the ordered search from n ~ 12 000 on (5.8x at
    // n = 50 000) and the query form from ~6000 queries on (1.9x at 10 000, 2.6x at 20 000 queries against 50 000 points; their
    // floor is one cold-started chunk scan, ~4 ms).
    // DGPAMD_NN_STORE_ONCE = 1 / 2 forces the store-once / the streaming kernels (the tests compare the two).
    const int force = (int)ctx->tune.nn_store_once;
    const bool pays = ordered ? nx >= 12000 : (nq >= 6000 && nx >= 20000);
    if (D <= 16 && m_out <= 64 && nx < INT_MAX && force != 1 && (pays || force == 2))
        return D <= 8 ? launch_nn_stream_k<8>(ctx, nq, nx, D, q, x, m_out, ordered, out)
                      : launch_nn_stream_k<16>(ctx, nq, nx, D, q, x, m_out, ordered, out);
    const unsigned grid = (unsigned)(nq < 2 * (int64_t)ctx->num_cu * 2 ? nq : 2 * (int64_t)ctx->num_cu * 2);
    double *scratch = nullptr;
    HIP_TRY(ctx, hipMallocAsync((void **)&scratch, (size_t)grid * nx * sizeof(double), ctx->stream));
    size_t shm = (D + 8 + NN_CMAX) * sizeof(double) + (NN_CMAX + 4 + (size_t)m_out) * sizeof(int64_t) + (NN_NB + 256 + 4) * sizeof(int);
    int rc = set_lds(ctx, (const void *)nn_select_big_kernel, shm);
    if (rc) return rc;
    hipLaunchKernelGGL(nn_select_big_kernel, dim3(grid), dim3(256), shm, ctx->stream, nq, nx, D, q, x, m_out, ordered, out, scratch);
    HIP_TRY(ctx, hipFreeAsync(scratch, ctx->stream));
    return DGPAMD_OK;
}

extern "C" int dgpamd_nn_ordered(dgpamd_ctx *ctx, int64_t n, int D, const double *x, int m, int64_t *NNarray) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || D <= 0 || !x || !NNarray || m < 0) BAD_ARG(ctx, "bad arguments");
    if (m > n - 1) m = (int)(n - 1);
    int rc = launch_nn(ctx, n, n, D, x, x, m + 1, 1, NNarray);
    if (rc) return rc;
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

__global__ void nn_cyclic_kernel(int64_t M, int m, int64_t *NN) {   // vecchia.py:23-26 (m == n shortcut)
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < M * m) NN[e] = ((e % m) + (e / m)) % m;
}

extern "C" int dgpamd_nn_query(dgpamd_ctx *ctx, int64_t M, int64_t n, int D, const double *q, const double *x, int m,
                               int64_t *NN) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (M <= 0 || n <= 0 || D <= 0 || !q || !x || !NN || m <= 0) BAD_ARG(ctx, "bad arguments");
    if (m >= n) {
        m = (int)n;
        hipLaunchKernelGGL(nn_cyclic_kernel, dim3((unsigned)((M * m + 255) / 256)), dim3(256), 0, ctx->stream, M, m, NN);
    } else {
        int rc = launch_nn(ctx, M, n, D, q, x, m, 0, NN);
        if (rc) return rc;
    }
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
