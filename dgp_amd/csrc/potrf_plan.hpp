// The host side of the dense factorisation, decided once: the task encoding of both kernels, the per-step tables
// (build_tasks) and the one-launch table (build_mega_tasks, mega_flatten), the plan of a one-launch call (mega_plan: panels
// per visit, queues, critical workers, groups, grid, the table's cache key) and the layout of the workspace.  potrf_step.hpp
// and potrf_mega.hpp upload and launch by it, dgpamd_potrf_workspace is sized from it, and tools/potrf_table_check.cpp
// walks every table it produces against the kernels' waits -- without a device.
// Plain C++17 (host arithmetic only): a host program includes it without HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/dgp_amd.h"
#include "tuning.hpp"

// ---- task encoding ------------------------------------------------------------------------------------------------------
// A task is a 64x64 tile update  C = (first ? 0 : C) +/- sum_{kb0 <= kb < kb0+nkb} L[li][kb] R[ri][kb]^T  (buffers A / T / S)
// followed by what `post` says (potrf_step.hpp, potrf_mega.hpp).
enum { T_STORE = 0, T_SOLVE = 1, T_CHAIN = 2, T_TDIAG = 3, T_LOOK = 4, T_LOOKD = 5 };
enum { BUF_A = 0, BUF_T = 1, BUF_S = 2 };

#define VER_FINAL 0x40000000   // version of a tile nobody will write again
#define VER_PLANES 4           // version words per matrix: buffers A, T, S + one plane of auxiliary words

// Four / two ints with the size, alignment and member offsets of HIP's int4 / int2 (the .hip files assert it): the tables are
// built here and uploaded as they stand.
struct alignas(16) Task4 {
    int32_t x, y, z, w;
};
struct alignas(8) Need2 {
    int32_t x, y;   // per block k: worker visits of A[k+1][k] and of A[k+1][k+1] the chain waits for
};
struct MegaTask {
    Task4 a;   // as the per-step tables: what / where (make_task)
    Task4 b;   // x: visits of the output tile before this one; y: bit 0 = this visit makes it final, bits 8.. = block step (critical queue);
               // z: block whose inverse a SOLVE / TDIAG / LOOK task multiplies with; w: LOOK / LOOKD: earlier visits of the tile it updates
};

static inline Task4 make_task(int post, int first, int plus, int mask_last, int bufC, int ci, int cj, int bufL, int li,
                              int bufR, int ri, int kb0, int nkb) {
    Task4 t;
    t.x = post | (first << 4) | (plus << 5) | (mask_last << 6) | (bufC << 8) | (bufL << 10) | (bufR << 12);
    t.y = ci | (cj << 16);
    t.z = li | (ri << 16);
    t.w = kb0 | (nkb << 16);
    return t;
}
// ... and back, field by field (host and device: both kernels decode with these, each where it needs the field)
constexpr int task_post(int x) { return x & 15; }
constexpr int task_first(int x) { return (x >> 4) & 1; }
constexpr int task_plus(int x) { return (x >> 5) & 1; }
constexpr int task_mask_last(int x) { return (x >> 6) & 1; }
constexpr int task_bufC(int x) { return (x >> 8) & 3; }
constexpr int task_bufL(int x) { return (x >> 10) & 3; }
constexpr int task_bufR(int x) { return (x >> 12) & 3; }
constexpr int task_lo(int v) { return v & 0xffff; }   // ci of y, li of z, kb0 of w
constexpr int task_hi(int v) { return v >> 16; }      // cj of y, ri of z, nkb of w

// ---- per-step tables (potrf_step_kernel): one vector of tasks per launch ----------------------------------------------------
#ifndef LAZY
#define LAZY 4   // panels (64-pivot blocks) applied per visit of a bulk tile
#endif
// ops: 64^3 multiply-add units per launch and matrix (for the profiler)
static inline void build_tasks(int nbk, bool inv, std::vector<std::vector<Task4>> &L, std::vector<double> &ops) {
    const int nl = nbk + (inv ? 2 : 0);
    L.assign(nl, {});
    ops.assign(nl, 0.0);
    for (int k = 0; k < nl; ++k) {
        std::vector<Task4> &t = L[k];
        double &w = ops[k];
        if (k < nbk) {
            const int np1 = k >= 1 ? 1 : 0;   // column k takes panel k-1 only
            t.push_back(make_task(T_CHAIN, 0, 0, 0, BUF_A, k, k, BUF_A, k, BUF_A, k, k - np1, np1));
            w += np1 + 1;
            if (inv) t.push_back(make_task(T_TDIAG, 1, 0, 0, BUF_T, k, k, BUF_A, 0, BUF_A, 0, 0, 0));
            for (int i = k + 1; i < nbk; ++i) {
                t.push_back(make_task(T_SOLVE, 0, 0, 0, BUF_A, i, k, BUF_A, i, BUF_A, k, k - np1, np1));
                w += np1 + 1;
            }
            if (inv)
                for (int q = k - 1; q >= 0; --q) {   // T[q][k]: first touched by panel k-1 when q == k-1
                    t.push_back(make_task(T_SOLVE, q == k - 1, 0, 0, BUF_T, q, k, BUF_T, q, BUF_A, k, k - 1, 1));
                    w += 2;
                }
            // lazy bulk of A: columns k+1, k+1+LAZY, ... take the LAZY panels (k-LAZY .. k-1)
            const int kb0 = k >= LAZY ? k - LAZY : 0, nkb = k - kb0;
            if (nkb > 0)
                for (int j = k + 1; j < nbk; j += LAZY)
                    for (int i = j; i < nbk; ++i) {
                        t.push_back(make_task(T_STORE, 0, 0, 0, BUF_A, i, j, BUF_A, i, BUF_A, j, kb0, nkb));
                        w += nkb;
                    }
            if (inv && nkb > 0)   // same rule for the rows of T that already have a panel: q <= k-1
                for (int j = k + 1; j < nbk; j += LAZY)
                    for (int q = 0; q <= k - 1; ++q) {
                        const int f0 = q > kb0 ? q : kb0;   // panels >= q only; the first visit starts from zero
                        t.push_back(make_task(T_STORE, f0 == q, 0, 0, BUF_T, q, j, BUF_T, q, BUF_A, j, f0, k - f0));
                        w += k - f0;
                    }
        }
        if (inv)   // S[q][q'] += Pt_q Pt_q'^T for the panels (k-2, k-1), rows q = k-2, k-4, ...
            for (int q = k - 2; q >= 0; q -= 2) {
                const int nkb = (k - 1 < nbk ? k : nbk) - (k - 2);   // clip to panels < nbk
                if (nkb <= 0) continue;
                const int mask = (k - 2 + nkb - 1 == nbk - 1) ? 1 : 0;   // the last block carries right-hand sides
                for (int q2 = 0; q2 <= q; ++q2) {
                    t.push_back(make_task(T_STORE, q == k - 2, 1, mask, BUF_S, q, q2, BUF_T, q, BUF_T, q2, k - 2, nkb));
                    w += nkb;
                }
            }
    }
}

// ---- task table of the one-launch kernel -------------------------------------------------------------------------
// The same right-looking schedule as build_tasks (lazy bulk: a tile takes LAZY panels per visit), restated per tile:
// `applied` panels so far, `visits` so far.  Differences: no chain tasks (the chain workgroups run on their own); the
// first panel tile A[k+1][k] gets its last worker visit as a plain update (the chain does the solve); what the chain
// waits for is produced one block step ahead of the rest (look-ahead, see below).
// Panels per visit of a trailing A / T tile and of a K^-1 tile, and where the cadence starts (see build_mega_tasks).  The
// per-step kernel's 4 / 2 / next column against 8 / 8 / three columns on gives potrf -12 % at 6 matrices and -13 % at 12,
// potrf_inv -19 % at 6: deeper visits run the tile engine at a higher rate, and a column whose last bulk visit lies three
// block steps before its solves does not have those solves queue up behind a 40-us task.
#define MEGA_LAZY 8
#define MEGA_SLAZY 8
#define MEGA_LAZY_CAP 24   // most panels per visit an override can ask for (a task waits on 1 + 2 nkb words with the 64 lanes of one wave)

// tag[i]: (block step << 1) | critical -- critical: the lane that hands the chain its next inputs (the look-ahead pair, the first solve
// of the panel column and the catch-up updates behind it); everything else is bulk.
static inline void build_mega_tasks(int nbk, bool inv, std::vector<MegaTask> &out, std::vector<Need2> &need, int lazy, int slazy,
                                    int near, int xcatch, int stail, int look, std::vector<int> &tag, int slag = 0) {
    int cur_step = 0, cur_urgent = 0;
    const int nb2 = nbk * nbk;
    std::vector<int> appliedA(nb2, 0), visitsA(nb2, 0), appliedT(nb2, 0), visitsT(nb2, 0), visitsS(nb2, 0), appliedS(nbk, 0);
    for (int q = 0; q < nbk; ++q) appliedS[q] = q;   // row q of K^-1 sums the panels kb >= q
    if (inv)
        for (int q = 0; q < nbk; ++q)
            for (int j = 0; j < nbk; ++j) appliedT[q * nbk + j] = q;   // T[q][j] sums the panels kb >= q
    need.assign(nbk, Need2{0, 0});
    auto emit = [&](Task4 a, int need_c, int fin, int wk) {
        MegaTask t;
        t.a = a;
        t.b = Task4{need_c, fin, wk, 0};
        out.push_back(t);
        tag.push_back((cur_step << 1) | (cur_urgent ? 1 : 0));
    };
    // bring A[i][j] up to the panels < upto (plain update, stored)
    auto updA = [&](int i, int j, int upto) {
        int &ap = appliedA[i * nbk + j];
        if (upto <= ap) return;
        emit(make_task(T_STORE, 0, 0, 0, BUF_A, i, j, BUF_A, i, BUF_A, j, ap, upto - ap), visitsA[i * nbk + j]++, 0, 0);
        ap = upto;
    };
    // bring T[q][j] up to the panels < upto
    auto updT = [&](int q, int j, int upto) {
        int &ap = appliedT[q * nbk + j];
        if (upto <= ap) return;
        emit(make_task(T_STORE, ap == q, 0, 0, BUF_T, q, j, BUF_T, q, BUF_A, j, ap, upto - ap), visitsT[q * nbk + j]++, 0, 0);
        ap = upto;
    };
    auto solveA = [&](int i, int k) {   // panel tile (i, k): the remaining updates, then the solve with W_k
        const int ap = appliedA[i * nbk + k];
        emit(make_task(T_SOLVE, 0, 0, 0, BUF_A, i, k, BUF_A, i, BUF_A, k, ap, k - ap), visitsA[i * nbk + k]++, 1, k);
        appliedA[i * nbk + k] = k;
    };
    // The look-ahead of block k as TWO tasks that run side by side, each with the solve of A[k+2][k] in it: T_LOOK applies
    // panel k to A[k+2][k+1], T_LOOKD stores the solved tile and applies panel k to A[k+2][k+2] (each tile lacks exactly that
    // panel: the catch-up tasks of block k-1 have brought them up to the panels < k).  One task for both left the diagonal
    // tile 4 us behind the panel tile, which the chain then waited for; and the solved tile is published by the task that has
    // time for it (the next block's catch-up tasks wait for it: published behind the panel-tile update it was 7 us late).
    auto lookA = [&](int k) -> bool {
        const int i = k + 2;
        if (!look || appliedA[i * nbk + k + 1] != k || appliedA[i * nbk + i] != k) return false;
        const int ap = appliedA[i * nbk + k];
        // T_LOOK first (it waits for nothing of T_LOOKD's; T_LOOKD waits for T_LOOK's "input read" word before it stores the
        // solved tile over the input): the table stays a topological order
        MegaTask t;
        t.a = make_task(T_LOOK, 0, 0, 0, BUF_A, i, k, BUF_A, i, BUF_A, k, ap, k - ap);
        t.b = Task4{visitsA[i * nbk + k], 0, k, visitsA[i * nbk + k + 1]};
        out.push_back(t);
        tag.push_back((cur_step << 1) | 1);
        MegaTask d;
        d.a = make_task(T_LOOKD, 0, 0, 0, BUF_A, i, k, BUF_A, i, BUF_A, k, ap, k - ap);
        d.b = Task4{visitsA[i * nbk + k]++, 1, k, visitsA[i * nbk + i]};
        out.push_back(d);
        tag.push_back((cur_step << 1) | 1);
        ++visitsA[i * nbk + k + 1];
        ++visitsA[i * nbk + i];
        appliedA[i * nbk + k] = k;
        appliedA[i * nbk + k + 1] = appliedA[i * nbk + i] = k + 1;
        return true;
    };
    const int nl = nbk + (inv ? 1 + slag : 0);   // (one more pass flushes what is left of K^-1)
    for (int k = 0; k < nl; ++k) {
        cur_step = k;
        if (k < nbk) {
            // LOOK-AHEAD: what the chain picks up after factoring block k+1 -- A[k+2][k+1] and A[k+2][k+2] with the panels
            // <= k -- needs only W_k and the chain's own panel tile A[k+1][k]: it comes first in the tasks of block k,
            // ahead of their bulk, so the chain's serial part (solve, update, factor: ~15 us) runs beside that bulk
            // instead of after it.
            if (k + 2 < nbk) {
                cur_urgent = 1;
                if (!lookA(k)) {
                    solveA(k + 2, k);
                    updA(k + 2, k + 2, k + 1);
                    updA(k + 2, k + 1, k + 1);
                }
                cur_urgent = 0;
                need[k + 1] = Need2{visitsA[(k + 2) * nbk + k + 1], visitsA[(k + 2) * nbk + k + 2]};
            }
            if (inv) emit(make_task(T_TDIAG, 1, 0, 0, BUF_T, k, k, BUF_A, 0, BUF_A, 0, 0, 0), visitsT[k * nbk + k]++, 1, k);
            // panel column k; behind its first tile the catch-up of the NEXT look-ahead's two tiles (panels <= k), so that
            // the visits the chain waits for apply one panel each
            for (int i = k + 3; i < nbk; ++i) {
                cur_urgent = (i == k + 3);
                solveA(i, k);
                cur_urgent = 0;
                if (i == k + 3) {
                    cur_urgent = 1;
                    updA(k + 3, k + 3, k + 1);
                    updA(k + 3, k + 2, k + 1);
                    if (xcatch) updA(k + 3, k + 1, k + 1);   // (the next look-ahead solve then has no panel left to apply)
                    // The next block's look-ahead tile A[k+3][k+1] up to the panels < k: all final by now.  The look-ahead tasks
                    // then apply ONE panel (k, whose operand the solve of A[k+3][k] publishes ~5 us before W_k+1) where they
                    // applied the three the lazy cadence leaves -- 5 us of arithmetic between the arrival of the last operand
                    // (the previous block's solved tile) and the solve, on the path to the tile the chain waits for.
                    else if (look) updA(k + 3, k + 1, k);
                    cur_urgent = 0;
                }
            }
            if (inv)
                for (int q = k - 1; q >= 0; --q) {
                    const int ap = appliedT[q * nbk + k];
                    emit(make_task(T_SOLVE, ap == q, 0, 0, BUF_T, q, k, BUF_T, q, BUF_A, k, ap, k - ap), visitsT[q * nbk + k]++, 1, k);
                    appliedT[q * nbk + k] = k;
                }
            // lazy bulk: columns k+1, k+1+LAZY, ... below the diagonal; diagonal tiles one block step ahead of that
            // (near: the cadence's first column is k+1+near -- a column's last bulk visit is then 1+near block steps before its
            //  solves, which do not queue up behind it.  The solves apply what is left: 1+near panels.)
            if (k > 0) {
                for (int j = k + 2 + near; j < nbk; j += lazy) updA(j, j, k);
                for (int j = k + 1 + near; j < nbk; j += lazy)
                    for (int i = j + 1; i < nbk; ++i) updA(i, j, k);
                if (inv)
                    for (int j = k + 1 + near; j < nbk; j += lazy)
                        for (int q = 0; q <= k - 1; ++q) updT(q, j, k);
            }
        }
        if (inv) {
            // S[q][q'] += Pt_q Pt_q'^T: row q is visited when `slazy` panels are pending (rows q = k - slazy, k - 2 slazy, ... at
            // block step k).  With `stail` (up to three matrices: the chains bound the time) the threshold shrinks towards the end
            // with the block steps that are left, so that when the last chain has finished every K^-1 tile lacks one or two
            // panels, not eight: the tail after the chains is one round of short tasks behind the last column's solves
            // (potrf_inv of one matrix 0.57 -> 0.55 ms, of three 0.77 -> 0.75; with more matrices the extra shallow tasks cost more than the tail).
            const int ks = k - slag;   // (slag: the K^-1 visits trail by that many block steps -- nothing waits for them)
            const int left = nbk - ks;   // block steps until the flush
            const int thr = ks >= nbk ? 1 : (stail && left < slazy ? (left > 1 ? left : 1) : slazy);
            for (int q = 0; q <= ks - 1 && q < nbk; ++q) {
                const int upto = ks < nbk ? ks : nbk;
                if (upto - appliedS[q] < thr) continue;
                const int ap = appliedS[q], nkb = upto - ap;
                const int mask = (upto - 1 == nbk - 1) ? 1 : 0;
                for (int q2 = 0; q2 <= q; ++q2)
                    emit(make_task(T_STORE, ap == q, 1, mask, BUF_S, q, q2, BUF_T, q, BUF_T, q2, ap, nkb), visitsS[q * nbk + q2]++, 0, 0);
                appliedS[q] = upto;
            }
        }
    }
}

// ---- the plan of one one-launch call ------------------------------------------------------------------------------------------
// Everything the host decides about a launch of potrf_mega_kernel, decided here and nowhere else.
// DGPAMD_MEGA_LAZY / _SLAZY / _NEAR / _LOOK / _SLAG / _QUEUES / _NCRIT / _GROUPS override (tuning only; the context's switches).
struct MegaKey {   // what the table depends on: the cache key of its device copy
    int v[9];      // nbk, inv, lazy, slazy, near, xcatch | stail << 1, look, queues, slag
    bool operator<(const MegaKey &o) const {
        for (int i = 0; i < 9; ++i)
            if (v[i] != o.v[i]) return v[i] < o.v[i];
        return false;
    }
};
struct MegaPlan {
    int nbk, inv, batch;
    int lazy, slazy;      // panels per visit of a trailing A / T tile and of a K^-1 tile (within MEGA_LAZY_CAP)
    int near;             // the lazy cadence starts 1 + near columns to the right of the chain
    int xcatch, stail;    // the catch-up of the next look-ahead solve's tile; the shrinking K^-1 threshold
    int look;             // 0: the look-ahead as three tasks (rounds 2-3)
    int slag;             // block steps by which the K^-1 visits trail
    int queues;           // 1: one queue per group of matrices; 2: critical + bulk
    int ncrit;            // workers per matrix that serve the critical queue first (MegaArgs::ncrit)
    int crit_per_xcd;     // ceil(ncrit x matrices / 8), at most 16: the critical-first workers per XCD the two-queue guard counts with
    int ngroups;          // groups the matrices and the XCDs are dealt into (MegaArgs::ngroups)
    int64_t slots;        // workgroups the device holds at once: wgs_per_cu x num_cu
    int wgs_per_cu;
    int64_t grid;         // workgroups of the launch; known once the table's length is (set_grid)
    MegaKey key;
    // every workgroup resident at once (not needed for progress, but a queued worker would only start late), and none without a task
    void set_grid(int ntask) {
        grid = slots;
        const int64_t useful = (int64_t)batch * (ntask + 1 + wgs_per_cu);
        if (grid > useful) grid = useful;
        if (grid < batch + 1) grid = batch + 1;
    }
};

static inline MegaPlan mega_plan(const Tuning &tn, int nbk, bool inv, int batch, int num_cu, int wgs_per_cu) {
    MegaPlan p;
    p.nbk = nbk; p.inv = inv ? 1 : 0; p.batch = batch;
    // Panels per visit: 8 (trailing and K^-1 tiles), 10 from six matrices on; the cadence starts three columns to the right
    // of the chain (near = 2).  Measured at n = 2000 (tools/gpu_lazy_sweep.py, profiles/r02_mega_table_sweeps.txt).
    const bool deep = batch >= 6;
    // (n = 5000, ten matrices with their inverses: 25.9 ms at 8 panels per visit, 25.3 at 12, 25.4 at 16 -- 49 TFLOP/s; one matrix is
    //  fastest at 8: the chain waits for deeper visits)
    // Round 4, with the 12.5-us chain (profiles/r04_mega_table_sweeps.txt, n = 2000): with the inverse, 10 panels per visit also
    // below six matrices (potrf_inv 0.610 -> 0.587 ms at two, 0.738 -> 0.714 at three, 0.813 -> 0.797 at four); from six on 12 panels
    // and the cadence starting one column further right (near = 3: 1.142 -> 1.124 ms at six, 1.977 -> 1.847 at ten).  Without
    // the inverse nothing moved (near = 3 costs one matrix 0.06 ms).
    const int deep_lazy = (nbk >= 64 || inv) ? 12 : 10;
    const int shallow = inv ? 10 : MEGA_LAZY, sshallow = inv ? 10 : MEGA_SLAZY;
    const int lazy = tn.mega_lazy ? (int)tn.mega_lazy : (deep ? deep_lazy : shallow), slazy = tn.mega_slazy ? (int)tn.mega_slazy : (deep ? deep_lazy : sshallow);
    // (a task waits on 1 + 2 nkb version words, one per lane of ONE wave: the overrides are clamped so that the deepest visit --
    //  lazy + 1 + near panels -- stays within 64 flags, and mega_flatten checks build_mega_tasks' output)
    p.lazy = lazy > MEGA_LAZY_CAP ? MEGA_LAZY_CAP : lazy;
    p.slazy = slazy > MEGA_LAZY_CAP ? MEGA_LAZY_CAP : slazy;
    // Round 5 (profiles/r05_mega_table_sweeps.txt): with the newest panel of a visit applied on its own (kernel, `split`) the solves can
    // leave more panels to themselves without lengthening the recursion along a row of tiles, and a column's last deep visit
    // then lies four block steps ahead of its solves: three columns' distance (near = 3) at every batch size.
    p.near = (int)tn.mega_near;
    p.xcatch = 0;
    p.stail = (inv && batch <= 3) ? 1 : 0;
    p.look = (int)tn.mega_look;
    p.slag = (int)tn.mega_slag;
    // (workers of the critical queue per matrix: one per task of a block step, and a few more while the engine has room)
    p.ncrit = tn.mega_ncrit ? (int)tn.mega_ncrit : (batch <= 4 ? 12 : 8);
    p.crit_per_xcd = (p.ncrit * batch + 7) / 8;
    if (p.crit_per_xcd > 16) p.crit_per_xcd = 16;
    p.wgs_per_cu = wgs_per_cu;
    p.slots = (int64_t)wgs_per_cu * num_cu;
    // Two queues (critical lane + bulk) up to three matrices, one from four on.  (Re-measured after the synchronisation block's words got lines of their own,
    // profiles/r05_mega_table_sweeps.txt: most of what the critical queue had gained at four and more matrices was that ITS head did not share the line of the W
    // counters -- with every word on its own line one queue is 1-5 % faster there, the two still 1.5-3 % at one to three.)
    p.queues = tn.mega_queues ? (int)tn.mega_queues : (batch <= 3 ? 2 : 1);
    // The two-queue form needs workers of BOTH kinds: the kernel makes the first 8 x crit_per_xcd workers critical-first and everybody else
    // bulk-first.  On a small or CU-masked device every worker would be critical-first, run ahead into later block steps and wait there for
    // bulk tiles that nobody pulls -- until the spin limit trips.  One queue then.  (The guard counts with the device's slots, not with
    // the launch's grid, which a short table caps below them: tools/potrf_table_check.cpp lists the shapes where the two disagree.)
    if (p.slots - batch < 2 * 8 * (int64_t)p.crit_per_xcd) p.queues = 1;
    {
        // (measured at n = 2000, tools/gpu_lazy_sweep.py: uneven groups are fine -- an XCD whose own queue has run out takes
        // from the others -- so odd batches use two groups as well: potrf_inv -10 % at 3 matrices, -7 % at 6, -12 % at 12)
        // (round 5, same sweeps: three matrices with the inverse, and odd batches without it, are 3-5 % faster as ONE group -- two groups of 2 + 1 or 3 + 2
        //  matrices leave half the XCDs with the smaller share until their queue runs out)
        const bool one_group = (batch & 1) && (batch == 3 || !inv);
        int G = tn.mega_groups ? (int)tn.mega_groups : (one_group ? 1 : batch % 8 == 0 ? 8 : batch % 4 == 0 ? 4 : batch >= 2 ? 2 : 1);
        while (G > batch) G >>= 1;
        p.ngroups = G;
    }
    p.grid = 0;
    p.key = MegaKey{{nbk, p.inv, p.lazy, p.slazy, p.near, p.xcatch | (p.stail << 1), p.look, p.queues, p.slag}};
    return p;
}

// The table as the kernel reads it: with two queues the critical tasks first (their block step rides in b.y above the `final`
// bit), then the bulk tasks; with one queue the builder's order.  What is uploaded and what the checker walks are these bytes.
struct MegaFlat {
    std::vector<MegaTask> tasks;   // nut critical tasks, then the bulk
    std::vector<Need2> need;       // chain_need, one per block
    int ntask = 0, nut = 0;
    bool refused = false;          // a visit applies more panels than one wave can wait for (1 + 2 nkb > 64): nothing to launch
};
static inline MegaFlat mega_flatten(const MegaPlan &p) {
    MegaFlat f;
    std::vector<MegaTask> all;
    std::vector<int> tag;
    build_mega_tasks(p.nbk, p.inv != 0, all, f.need, p.lazy, p.slazy, p.near, p.xcatch, p.stail, p.look, tag, p.slag);
    for (const MegaTask &t : all)   // wg_wait_flags polls with the 64 lanes of one wave
        if (1 + 2 * task_hi(t.a.w) > 64) f.refused = true;
    if (p.queues == 2)
        for (size_t i = 0; i < all.size(); ++i)
            if (tag[i] & 1) {
                MegaTask t = all[i];
                t.b.y |= (tag[i] >> 1) << 8;
                f.tasks.push_back(t);
            }
    f.nut = (int)f.tasks.size();
    for (size_t i = 0; i < all.size(); ++i)
        if (p.queues != 2 || !(tag[i] & 1)) f.tasks.push_back(all[i]);
    f.ntask = (int)f.tasks.size();
    return f;
}

// ---- the synchronisation block of the one-launch kernel and the workspace layout ----------------------------------------------
// One word on a 128-byte line of its own.  Round 5: the queue heads (one returning atomic per task pulled), the status word and the first sixteen matrices' W_k
// counters used to share ONE line -- every publication of a W_k by a chain queued behind the workers' ticket atomics and the polls of everyone who waited for any
// matrix's W (the "hot line" effects of profiles/r05_mega_table_sweeps.txt: one more read per solve of that line cost 15 %).
struct alignas(128) MegaLine {
    int32_t v;
    int32_t fill[31];
};
struct MegaSync {   // zeroed by a memset node ahead of every launch; the version words follow it
    int32_t pad0;                   // (padding)
    int32_t status;                 // 0, or the code of the first spin that gave up
    int32_t pad[30];                // (pad[0]: the spare word of the deferred post-processing)
    MegaLine ghead[8];              // queue head of each group of matrices (see MegaArgs::ngroups)
    MegaLine uhead[8];              // head of each group's CRITICAL queue (ghead: the bulk queue's), see MegaArgs::nut
    int32_t cukey[DGPAMD_MAXB];     // per matrix: CU of its chain workgroup (cu_key()); read once by every worker
    MegaLine wflag[DGPAMD_MAXB];    // per matrix: blocks factored (W_k is readable for k < wflag)
};
static_assert(sizeof(MegaSync) % 128 == 0, "MegaSync is whole lines");

// The workspace of dgpamd_potrf / dgpamd_potrf_inv, in this order: the diagonal-block inverses W_k (batch x nbk x 4096 doubles),
// {logdet (loglik), logdet (graph)} scratch (2 x DGPAMD_MAXB doubles), then info, step flags and chain CU keys of the per-step kernel
// (3 x DGPAMD_MAXB words), the one-launch kernel's synchronisation block (on a 128-byte line), its pivot array (batch x Np doubles).
static inline size_t potrf_ws_doubles(int64_t n, int batch) {
    int64_t nbk = padded_dim(n) / 64;
    return (size_t)batch * nbk * 4096 + 2 * DGPAMD_MAXB;   // diagonal inverses + {logdet (loglik), logdet (graph)} scratch; info words follow
}
// bytes of the one-launch kernel's synchronisation block (MegaSync + tile versions), a multiple of 16
static inline size_t mega_sync_bytes(int64_t nbk, int batch) {
    size_t b = sizeof(MegaSync) + (size_t)batch * VER_PLANES * nbk * nbk * sizeof(int32_t);
    return (b + 15) / 16 * 16;
}
// offset of the one-launch kernel's synchronisation block inside the workspace (on a 128-byte line: its hot words have lines of their own)
static inline size_t mega_sync_offset(int64_t n, int batch) {
    const size_t b = potrf_ws_doubles(n, batch) * sizeof(double) + 3 * DGPAMD_MAXB * sizeof(int32_t);   // + info, step flags, chain CU keys
    return (b + 127) / 128 * 128;
}
// offset of the one-launch kernel's pivot array (batch x Np doubles) behind the synchronisation block
static inline size_t mega_piv_offset(int64_t n, int batch) {
    return mega_sync_offset(n, batch) + mega_sync_bytes(padded_dim(n) / 64, batch);
}
static inline size_t potrf_workspace_bytes(int64_t n, int batch) {
    return mega_piv_offset(n, batch) + (size_t)batch * padded_dim(n) * sizeof(double);
}

#ifdef __HIPCC__
// The library is built without relocatable device code: each kernel is launched from the file it lives in.
struct dgpamd_ctx;
// potrf_step.hpp: the per-step tables on the device (uploaded on first use, with the kernel's occupancy query: both outside a
// graph capture), and one launch per block step
struct TaskTable;
int get_tasks(dgpamd_ctx *ctx, int nbk, bool inv, TaskTable *&out);
int potrf_launches(dgpamd_ctx *ctx, int64_t n, double *A, double *T, double *S, int64_t stride_a, int batch, double *logdet,
                   int32_t *info, double *ws, int32_t *flags, const TaskTable *tt);
// potrf_mega.hpp: plan, table (uploaded on first use) and the one launch; the synchronisation block and the pivots lie in `ws`
// where the layout above says
int potrf_mega_launch(dgpamd_ctx *ctx, int64_t n, double *A, double *T, double *S, int64_t stride_a, int batch, double *logdet,
                      int32_t *info, double *ws, bool sync_cleared);
#endif
