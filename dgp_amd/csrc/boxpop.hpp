// What the per-draw steps of the population methods over one box share (boxsmc.hip's TEMPER, DESIGN I.21; boxsus.hip's LEVEL,
// DESIGN I.22), every shared step written once: the workgroup of a draw, the reduction over it, the scan over a thread's chunk,
// the gather of the chosen particles into x_trial, and on the host the size check and the launch.
//
// P draws with R particles each, Q = P R lanes q = p R + r; one workgroup per draw, its R particles the parallelism.  The
// threads of a draw are min(1024, R rounded up to 64), fixed by R, and every order of additions below is fixed by them: a
// draw's numbers do not depend on P or on the other draws of the launch.  What selects the particles -- TEMPER's bisection and
// systematic resampling, LEVEL's keys, radix select and spread -- stays in its own file.  Everything on the device is forced
// inline, as in boxchain.hpp and wave.hpp: a kernel compiles to what it did with a copy of its own.
#pragma once
#include "common.hpp"

static_assert(DGPAMD_BOXSMC_MAXR == DGPAMD_BOXSUS_MAXR, "the two per-draw steps share their workgroup and its scratch");
#define BOXPOP_THREADS 1024
#define BOXPOP_WAVES (BOXPOP_THREADS / 64)

static unsigned boxpop_threads(int64_t R) { return (unsigned)(R >= BOXPOP_THREADS ? BOXPOP_THREADS : (R + 63) / 64 * 64); }

// A thread's place in its draw's workgroup: thread t of NT, lane `lane` of wave w of NW
struct BoxpopThread {
    int t, NT, lane, w, NW;
};
__device__ __forceinline__ BoxpopThread boxpop_thread() {
    const int t = threadIdx.x, NT = blockDim.x;
    return BoxpopThread{t, NT, t & 63, t >> 6, NT >> 6};
}

struct BoxpopAdd {
    template <class T>
    static __device__ __forceinline__ T of(T a, T b) { return a + b; }
};
struct BoxpopMax {
    static __device__ __forceinline__ double of(double a, double b) { return fmax(a, b); }
};

// (v1, v2) <- Op over the workgroup of the values the threads bring (each its lane-strided partial), in every thread: the xor
// butterfly of the wave, 32 .. 1 (both partners combine the same two numbers), then the NW wave totals in index order.  N = 1:
// v2 is not touched.  buf: one of the two halves of the scratch, used in turn by the caller, so that one barrier per call is
// enough: who still reads the totals of call n has not passed the barrier of call n + 1, so nobody stores those of call n + 2.
template <class Op, int N, class T>
__device__ __forceinline__ void boxpop_reduce(const BoxpopThread &th, T (*buf)[BOXPOP_WAVES], T &v1, T &v2) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v1 = Op::of(v1, __shfl_xor(v1, off, 64));
        if (N == 2) v2 = Op::of(v2, __shfl_xor(v2, off, 64));
    }
    if (th.lane == 0) {
        buf[0][th.w] = v1;
        if (N == 2) buf[1][th.w] = v2;
    }
    __syncthreads();
    v1 = buf[0][0];
    if (N == 2) v2 = buf[1][0];
    for (int v = 1; v < th.NW; ++v) {
        v1 = Op::of(v1, buf[0][v]);
        if (N == 2) v2 = Op::of(v2, buf[1][v]);
    }
}
template <class Op, class T>
__device__ __forceinline__ T boxpop_reduce(const BoxpopThread &th, T (*buf)[BOXPOP_WAVES], T v) {
    boxpop_reduce<Op, 1>(th, buf, v, v);
    return v;
}

// The exclusive scan of term(i), i = 0 .. R - 1, in three levels: a thread sums its chunk [i0, i1) in index order (run), a
// lane's offset L is the sum of the totals of the lanes before it in its wave, one after the other, a wave's offset B likewise
// over the waves, so the value before particle i0 is B + L and the one after a chunk B + (L + run): each level's last value
// is the next one's first offset, by the same additions.  TOTAL: also total, the sum over the workgroup, which LEVEL needs.
// (Chosen at compile time and the loop over the waves written twice: with the one loop to NW and a total that TEMPER leaves
// unused, the compiler laid TEMPER's resampling blocks out behind the lanes' loop instead of before it -- the same
// instructions in another order.)  tot (BOXPOP_THREADS) and wtot (BOXPOP_WAVES): scratch; two barriers.
template <class T>
struct BoxpopScan {
    int i0, i1;
    T run, L, B, total;
};
template <bool TOTAL, class T, class Term>
__device__ __forceinline__ BoxpopScan<T> boxpop_scan(const BoxpopThread &th, int R, T *tot, T *wtot, Term term) {
    BoxpopScan<T> s;
    const int chunk = (R + th.NT - 1) / th.NT;
    s.i0 = min(th.t * chunk, R), s.i1 = min(s.i0 + chunk, R);
    s.run = 0;
    for (int i = s.i0; i < s.i1; ++i) s.run = s.run + term(i);
    tot[th.t] = s.run;
    __syncthreads();
    s.L = 0;
    for (int j = 0; j < 63; ++j)
        if (j < th.lane) s.L = s.L + tot[th.w * 64 + j];
    if (th.lane == 63) wtot[th.w] = s.L + s.run;
    __syncthreads();
    s.B = 0, s.total = 0;
    if (TOTAL) {
        for (int v = 0; v < th.NW; ++v) {
            const T c = wtot[v];
            if (v < th.w) s.B = s.B + c;
            s.total = s.total + c;
        }
    } else {
        for (int v = 0; v < th.w; ++v) s.B = s.B + wtot[v];
    }
    return s;
}

// GATHER: slot j of the draw gets particle anc(j), read from the moves' state x (D x Q) and written to the trial array
template <class Anc>
__device__ __forceinline__ void boxpop_gather(const BoxpopThread &th, int R, int D, int64_t Q, int64_t q0, const double *x,
                                              double *x_trial, Anc anc) {
    for (int64_t e = th.t; e < (int64_t)R * D; e += th.NT) {
        const int64_t j = e / D, d = e - j * D;
        x_trial[(q0 + j) * D + d] = x[d * Q + q0 + anc((int)j)];
    }
}
// the particles stay: anc[i] = i and its gather
__device__ __forceinline__ void boxpop_stay(const BoxpopThread &th, int R, int D, int64_t Q, int64_t q0, const double *x,
                                            double *x_trial, int32_t *anc) {
    for (int i = th.t; i < R; i += th.NT) anc[i] = i;
    boxpop_gather(th, R, D, Q, q0, x, x_trial, [](int j) { return j; });
}

// The sizes a per-draw step takes, and the refusal of the others under the entry point's own name for R's bound
static bool boxpop_sizes(int64_t P, int64_t R, int D) {
    return P >= 1 && R >= 1 && R <= DGPAMD_BOXSMC_MAXR && P <= 0x7fffffffLL / R && D >= 1 && D <= DGPAMD_MAXD;
}
#define BOXPOP_SIZES(MAXR) "need P >= 1, 1 <= R <= " MAXR ", P R < 2^31 and 1 <= D <= DGPAMD_MAXD"

// The launch of a per-draw step: shm bytes of dynamic LDS, the count of the draws that go on zeroed, one workgroup per draw
template <class Args>
static int boxpop_launch(dgpamd_ctx *ctx, void (*kernel)(Args), const Args &a, int64_t P, int64_t R, size_t shm, int32_t *running) {
    const int rc = set_lds(ctx, (const void *)kernel, shm);
    if (rc != DGPAMD_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(running, 0, sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(kernel, dim3((unsigned)P), dim3(boxpop_threads(R)), shm, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
