// The host side of the dense factorisation (csrc/potrf_plan.hpp: task tables, the plan of a one-launch call, the workspace
// layout) over a grid of shapes and switches, under AddressSanitizer / UBSan, without a device and without HIP.
//
// The kernels' waits are restated here, independently of the table builders, from the wait sites of the worker loop and of the
// chain (csrc/potrf_mega.hpp: potrf_mega_kernel, mega_chain2), and every flattened table is WALKED: one in-order puller per queue
// plus the chain, each advancing only when the wait its head stands at holds.
//   worker   waits until its output tile's version is b.x and every operand tile (bufL, li, kb), (bufR, ri, kb), kb0 <= kb <
//            kb0 + nkb, is final; T_STORE then publishes b.x + 1 (VER_FINAL with b.y bit 0).  T_TDIAG waits for W_wk only.
//            T_SOLVE / T_LOOK / T_LOOKD then wait for W_wk.  T_LOOK sets the tile's auxiliary word behind its first wait, then
//            waits for A[ci-1][cj] final and for A[ci][cj+1] at b.w, and publishes that tile at b.w + 1.  T_LOOKD waits for
//            A[ci][ci] at b.w and for the auxiliary word, publishes its own tile final and the diagonal tile at b.w + 1.
//   chain    block k: publishes W_k; needs A[k+1][k] and A[k+1][k+1] at exactly chain_need[k]; makes A[k+1][k] final.
// Asserted per table: the walk drains every queue and finishes the chain, in three orders of who moves first (the kernel's
// "topological order" claim, for one queue and for two); no version a waiter finds differs from the one it names; every A tile
// takes the panels [0, k) once each in ascending order before its solve or pick-up, T[q][j] the panels [q, j), S[q][q2] the
// panels [q, nbk); `first` exactly on the visit that starts from zero, `mask_last` exactly on the visit that holds panel nbk-1;
// at the end every A tile below the diagonal and every T tile is final; 1 + 2 nkb <= 64 or the flattening refused the table.
// Per plan: grid >= batch + 1, groups in {1, 2, 4, 8} and <= batch, critical workers per XCD <= 16, ncrit and queues as the two
// former sites computed them, the workspace offsets ascending and aligned.  The per-step tables (build_tasks) are held to the
// same coverage statements.  Printed, not asserted: the shapes where the two-queue guard's premise (the device's workgroup
// slots) and the launch's real grid disagree.
// Build and run on a CPU (from the repository root):
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/potrf_table_check.cpp -o build/potrf_table_check
//   build/potrf_table_check                      (the whole grid)
//   build/potrf_table_check --dump nbk inv batch (the flattened table of the default switches on 256 CUs x 2 workgroups: one
//                                                 task per line as its eight ints, then chain_need, two ints per line)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <string>

#include "../dgp_amd/csrc/potrf_plan.hpp"

static int failures = 0;
static long long tables = 0, plans = 0, tasks_walked = 0;
static std::string where;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond) && ++failures <= 30) printf("FAIL %s [%s]\n", #cond, where.c_str()); \
    } while (0)

static Tuning default_tuning() {   // context.hip's table: the built-in values of the switches the plan reads
    Tuning tn;
    memset(&tn, 0, sizeof(tn));
    tn.potrf_mode = 1;
    tn.mega_near = 3;
    tn.mega_look = 1;
    tn.mega_split = 1;
    return tn;
}

// panels applied so far to every tile of A, T (T[q][j] starts at q) and S (S[q][q2] starts at q)
struct Cover {
    int nbk;
    std::vector<int> ap[3];
    Cover(int nbk_) : nbk(nbk_) {
        for (auto &v : ap) v.assign((size_t)nbk * nbk, 0);
        for (int q = 0; q < nbk; ++q)
            for (int j = 0; j < nbk; ++j) ap[BUF_T][q * nbk + j] = ap[BUF_S][q * nbk + j] = q;
    }
    int &at(int buf, int i, int j) { return ap[buf][(size_t)i * nbk + j]; }
    void visit(int buf, int i, int j, int kb0, int nkb) {   // the panels [kb0, kb0 + nkb), once each, in ascending order
        if (nkb == 0) return;
        CHECK(at(buf, i, j) == kb0);
        at(buf, i, j) = kb0 + nkb;
    }
};

// what a task's words must say whatever the schedule: ranges, operands of its buffer, first / plus / mask_last, the wave limit
static void check_fields(const Task4 &a, int nbk, bool refused) {
    const int post = task_post(a.x), bufC = task_bufC(a.x), bufL = task_bufL(a.x), bufR = task_bufR(a.x);
    const int ci = task_lo(a.y), cj = task_hi(a.y), li = task_lo(a.z), ri = task_hi(a.z), kb0 = task_lo(a.w), nkb = task_hi(a.w);
    CHECK(ci < nbk && cj < nbk && li < nbk && ri < nbk && nkb >= 0 && kb0 + nkb <= nbk);
    CHECK(1 + 2 * nkb <= 64 || refused);
    CHECK(task_mask_last(a.x) == (nkb > 0 && kb0 + nkb == nbk ? 1 : 0));
    CHECK(task_plus(a.x) == (bufC == BUF_S ? 1 : 0));
    if (post == T_TDIAG) {
        CHECK(bufC == BUF_T && ci == cj && nkb == 0 && task_first(a.x) == 1);
        return;
    }
    if (bufC == BUF_A) {   // A[ci][cj] -= A[ci][kb] A[cj][kb]^T, kb < cj <= ci
        CHECK(bufL == BUF_A && bufR == BUF_A && li == ci && ri == cj && cj <= ci && kb0 + nkb <= cj && task_first(a.x) == 0);
    } else if (bufC == BUF_T) {   // T[q][j] -= T[q][kb] A[j][kb]^T, q <= kb < j
        CHECK(bufL == BUF_T && bufR == BUF_A && li == ci && ri == cj && ci < cj && kb0 >= ci && kb0 + nkb <= cj && post != T_LOOK && post != T_LOOKD);
        CHECK(task_first(a.x) == (kb0 == ci ? 1 : 0));
    } else {   // S[q][q2] += T[q][kb] T[q2][kb]^T, kb >= q >= q2
        CHECK(bufC == BUF_S && bufL == BUF_T && bufR == BUF_T && li == ci && ri == cj && cj <= ci && kb0 >= ci && nkb > 0 && post == T_STORE);
        CHECK(task_first(a.x) == (kb0 == ci ? 1 : 0));
    }
}

// ---- the one-launch table: the walk -------------------------------------------------------------------------------------------
struct Walk {
    const MegaFlat &f;
    const int nbk, inv;
    std::vector<int> ver[VER_PLANES];   // A, T, S, auxiliary words
    std::vector<char> pair_seen;        // the solve of a T_LOOK / T_LOOKD pair has been counted
    Cover cov;
    int wflag = 0;                      // blocks factored
    int head[2], end[2], stage[2] = {0, 0};
    int ck = 0, cstage = 0;             // the chain: block, stage; cstage 3: done
    Walk(const MegaFlat &f_, int nbk_, int inv_) : f(f_), nbk(nbk_), inv(inv_), pair_seen((size_t)nbk_ * nbk_, 0), cov(nbk_) {
        for (auto &v : ver) v.assign((size_t)nbk * nbk, 0);
        head[0] = 0; end[0] = f.nut; head[1] = f.nut; end[1] = f.ntask;
    }
    int &v(int plane, int i, int j) { return ver[plane][(size_t)i * nbk + j]; }
    // a wait for `need`: holds from need on (the kernel compares >=); a holder other than need itself is an overshoot
    bool reached(int plane, int i, int j, int need) {
        const int got = v(plane, i, j);
        if (got < need) return false;
        CHECK(got == need);
        return true;
    }
    // one step of queue q's head task; false: its wait does not hold
    bool worker(int q) {
        const MegaTask &t = f.tasks[head[q]];
        const Task4 &a = t.a;
        const int post = task_post(a.x), bufC = task_bufC(a.x), bufL = task_bufL(a.x), bufR = task_bufR(a.x);
        const int ci = task_lo(a.y), cj = task_hi(a.y), li = task_lo(a.z), ri = task_hi(a.z), kb0 = task_lo(a.w), nkb = task_hi(a.w);
        const int need_c = t.b.x, fin = t.b.y & 1, wk = t.b.z, need2 = t.b.w;
        const int newver = fin ? VER_FINAL : need_c + 1;
        int &st = stage[q];
        auto done = [&]() { st = 0; ++head[q]; ++tasks_walked; return true; };
        if (post == T_TDIAG) {
            if (wflag < wk + 1) return false;
            CHECK(wk == ci && v(bufC, ci, cj) == need_c && fin);
            v(bufC, ci, cj) = newver;
            return done();
        }
        if (st == 0) {
            if (!reached(bufC, ci, cj, need_c)) return false;
            for (int kb = kb0; kb < kb0 + nkb; ++kb)
                if (v(bufL, li, kb) != VER_FINAL || v(bufR, ri, kb) != VER_FINAL) return false;
            if (post == T_LOOK || post == T_LOOKD) {   // the pair's solve of A[ci][cj]: the same visit, computed by both
                char &seen = pair_seen[(size_t)ci * nbk + cj];
                if (!seen) cov.visit(bufC, ci, cj, kb0, nkb);
                else CHECK(cov.at(bufC, ci, cj) == kb0 + nkb);
                seen = 1;
            } else
                cov.visit(bufC, ci, cj, kb0, nkb);
            if (post == T_STORE) {
                CHECK(!fin);
                v(bufC, ci, cj) = newver;
                return done();
            }
            if (post == T_LOOK) v(3, ci, cj) = 1;   // (acc holds everything this task reads of the tile)
            st = 1;
            return true;
        }
        if (st == 1) {   // T_SOLVE / T_LOOK / T_LOOKD: W_wk, with every panel < cj applied
            if (wflag < wk + 1) return false;
            CHECK(wk == cj && cov.at(bufC, ci, cj) == cj);
            if (post == T_SOLVE) {
                CHECK(fin);
                v(bufC, ci, cj) = newver;
                return done();
            }
            CHECK(bufC == BUF_A && ci == cj + 2);
            st = 2;
            return true;
        }
        if (post == T_LOOK) {   // Q = A[ci][cj+1] -= S P^T, P = A[ci-1][cj]: the chain's panel tile
            if (v(BUF_A, ci - 1, cj) != VER_FINAL || !reached(BUF_A, ci, cj + 1, need2)) return false;
            CHECK(!fin);
            cov.visit(BUF_A, ci, cj + 1, cj, 1);
            v(BUF_A, ci, cj + 1) = need2 + 1;
            return done();
        }
        CHECK(post == T_LOOKD);   // the solved tile, final; D = A[ci][ci] -= S S^T
        if (!reached(BUF_A, ci, ci, need2) || v(3, ci, cj) < 1) return false;
        CHECK(fin);
        v(BUF_A, ci, cj) = newver;
        cov.visit(BUF_A, ci, ci, cj, 1);
        v(BUF_A, ci, ci) = need2 + 1;
        return done();
    }
    bool chain() {
        if (cstage == 3) return false;
        if (cstage == 0) {   // block ck factored (its diagonal tile: every panel < ck applied, the last one by the chain itself)
            wflag = ck + 1;
            cstage = ck + 1 == nbk ? 3 : 1;
            return true;
        }
        const Need2 need = f.need[ck];
        if (cstage == 1) {
            if (!reached(BUF_A, ck + 1, ck, need.x)) return false;
            CHECK(cov.at(BUF_A, ck + 1, ck) == ck);
            cstage = 2;
            return true;
        }
        if (!reached(BUF_A, ck + 1, ck + 1, need.y)) return false;
        CHECK(cov.at(BUF_A, ck + 1, ck + 1) == ck);
        cov.visit(BUF_A, ck + 1, ck + 1, ck, 1);   // D -= P P^T
        v(BUF_A, ck + 1, ck) = VER_FINAL;
        ++ck;
        cstage = 0;
        return true;
    }
    // order: which of the three actors moves first; each moves as far as it can before the next one is asked
    void run(int order) {
        for (bool progress = true; progress;) {
            progress = false;
            for (int s = 0; s < 3; ++s) {
                const int actor = (s + order) % 3;
                if (actor == 2)
                    while (chain()) progress = true;
                else
                    while (head[actor] < end[actor] && worker(actor)) progress = true;
            }
        }
        CHECK(head[0] == end[0] && head[1] == end[1] && cstage == 3);   // liveness
        if (head[0] != end[0] || head[1] != end[1] || cstage != 3) return;
        for (int i = 0; i < nbk; ++i)
            for (int j = 0; j < nbk; ++j) {
                if (j < i) CHECK(v(BUF_A, i, j) == VER_FINAL && cov.at(BUF_A, i, j) == j);
                if (j == i) CHECK(cov.at(BUF_A, i, i) == i);
                if (inv && j >= i) CHECK(v(BUF_T, i, j) == VER_FINAL && cov.at(BUF_T, i, j) == j);
                if (inv && j <= i) CHECK(cov.at(BUF_S, i, j) == nbk);
            }
    }
};

static void check_mega_table(const MegaPlan &p) {
    const MegaFlat f = mega_flatten(p);
    ++tables;
    CHECK(f.ntask == (int)f.tasks.size() && f.nut >= 0 && f.nut <= f.ntask && (int)f.need.size() == p.nbk);
    CHECK((p.queues == 2) == (f.nut > 0) || f.ntask == 0 || p.nbk < 3);
    CHECK(!f.refused);   // (the clamps of the switches keep every visit within one wave's flags)
    for (int i = 0; i < f.ntask; ++i) {
        check_fields(f.tasks[i].a, p.nbk, f.refused);
        CHECK(task_post(f.tasks[i].a.x) != T_CHAIN);
        if (i >= f.nut) CHECK((f.tasks[i].b.y >> 8) == 0);
        if (i > 0 && i < f.nut) CHECK((f.tasks[i].b.y >> 8) >= (f.tasks[i - 1].b.y >> 8));   // the critical queue: by block step
    }
    for (int order = 0; order < 3; ++order) Walk(f, p.nbk, p.inv).run(order);
}

// ---- the per-step tables: launch k's tasks run side by side, the launches in order ------------------------------------------------
static void check_step_tables(int nbk, bool inv) {
    std::vector<std::vector<Task4>> L;
    std::vector<double> ops;
    build_tasks(nbk, inv, L, ops);
    ++tables;
    CHECK((int)L.size() == nbk + (inv ? 2 : 0) && ops.size() == L.size());
    Cover cov(nbk);
    std::vector<int> fin[3];   // launch that made the tile final, or a large number
    for (auto &v : fin) v.assign((size_t)nbk * nbk, 1 << 30);
    for (int k = 0; k < (int)L.size(); ++k) {
        std::set<int> written;
        double units = 0.0;
        for (const Task4 &a : L[k]) {
            check_fields(a, nbk, false);
            const int post = task_post(a.x), bufC = task_bufC(a.x), bufL = task_bufL(a.x), bufR = task_bufR(a.x);
            const int ci = task_lo(a.y), cj = task_hi(a.y), li = task_lo(a.z), ri = task_hi(a.z), kb0 = task_lo(a.w), nkb = task_hi(a.w);
            CHECK(written.insert((bufC * nbk + ci) * nbk + cj).second);   // one task per tile and launch
            CHECK(post != T_LOOK && post != T_LOOKD);
            for (int kb = kb0; kb < kb0 + nkb; ++kb)   // operands: final since an earlier launch
                CHECK(fin[bufL][(size_t)li * nbk + kb] < k && fin[bufR][(size_t)ri * nbk + kb] < k);
            cov.visit(bufC, ci, cj, kb0, nkb);
            units += post == T_TDIAG ? 0 : (post == T_STORE ? nkb : nkb + 1);
            if (post == T_CHAIN) CHECK(bufC == BUF_A && ci == k && cj == k && cov.at(BUF_A, k, k) == k);
            if (post == T_TDIAG) CHECK(ci == k);
            if (post == T_SOLVE) CHECK(cj == k && cov.at(bufC, ci, cj) == k);
            if (post != T_STORE) fin[bufC][(size_t)ci * nbk + cj] = k;
        }
        CHECK(units == ops[k]);
    }
    for (int i = 0; i < nbk; ++i)
        for (int j = 0; j < nbk; ++j) {
            if (j <= i) CHECK(fin[BUF_A][(size_t)i * nbk + j] == j && cov.at(BUF_A, i, j) == j);
            if (inv && j >= i) CHECK(fin[BUF_T][(size_t)i * nbk + j] == j && cov.at(BUF_T, i, j) == j);
            if (inv && j <= i) CHECK(cov.at(BUF_S, i, j) == nbk);
        }
}

// ---- the plan and the workspace ------------------------------------------------------------------------------------------------
static std::map<std::string, std::set<int>> premise;   // "inv batch" -> nbk where the guard's premise and the real grid disagree

static void check_plan(const Tuning &tn, int nbk, bool inv, int batch, int num_cu, int wgs, bool defaults) {
    ++plans;
    MegaPlan p = mega_plan(tn, nbk, inv, batch, num_cu, wgs);
    // as get_mega_tasks and potrf_mega_launch computed them
    const int ncrit = tn.mega_ncrit ? (int)tn.mega_ncrit : (batch <= 4 ? 12 : 8);
    int crit = (ncrit * batch + 7) / 8;
    if (crit > 16) crit = 16;
    int queues = tn.mega_queues ? (int)tn.mega_queues : (batch <= 3 ? 2 : 1);
    if ((int64_t)wgs * num_cu - batch < 2 * 8 * (int64_t)crit) queues = 1;
    CHECK(p.ncrit == ncrit && p.crit_per_xcd == crit && p.crit_per_xcd <= 16 && p.queues == queues);
    CHECK(p.lazy >= 1 && p.lazy <= MEGA_LAZY_CAP && p.slazy >= 1 && p.slazy <= MEGA_LAZY_CAP);
    CHECK((p.ngroups == 1 || p.ngroups == 2 || p.ngroups == 4 || p.ngroups == 8) && p.ngroups <= batch);
    static std::map<MegaKey, int> ntask_of;   // the table depends on the key only: walked once per key
    auto it = ntask_of.find(p.key);
    if (it == ntask_of.end()) {
        check_mega_table(p);
        it = ntask_of.emplace(p.key, mega_flatten(p).ntask).first;
    }
    p.set_grid(it->second);
    CHECK(p.grid >= batch + 1 && p.grid <= (p.slots > batch + 1 ? p.slots : batch + 1));
    if (defaults && p.queues == 2 && p.grid - batch < 16 * (int64_t)crit)   // (the guard let two queues through; by the grid it would not)
        premise[std::to_string(inv) + " " + std::to_string(batch)].insert(nbk);
    // the workspace: W_k and the scratch doubles, three arrays of words, the synchronisation block on a line, the pivots
    for (int64_t n : {(int64_t)nbk * 64 - 64, (int64_t)nbk * 64 - 1}) {
        if (n < 1) continue;
        CHECK(padded_dim(n) == (int64_t)nbk * 64);
        const size_t words = potrf_ws_doubles(n, batch) * sizeof(double), so = mega_sync_offset(n, batch), po = mega_piv_offset(n, batch);
        CHECK(words == ((size_t)batch * nbk * 4096 + 2 * DGPAMD_MAXB) * sizeof(double));
        CHECK(so >= words + 3 * DGPAMD_MAXB * sizeof(int32_t) && so % 128 == 0 && so - words < 3 * DGPAMD_MAXB * sizeof(int32_t) + 128);
        CHECK(po == so + mega_sync_bytes(nbk, batch) && po % sizeof(double) == 0);
        CHECK(mega_sync_bytes(nbk, batch) >= sizeof(MegaSync) + (size_t)batch * VER_PLANES * nbk * nbk * sizeof(int32_t));
        CHECK(potrf_workspace_bytes(n, batch) == po + (size_t)batch * nbk * 64 * sizeof(double));
    }
}

static int dump(int nbk, int inv, int batch) {
    MegaPlan p = mega_plan(default_tuning(), nbk, inv != 0, batch, 256, 2);
    const MegaFlat f = mega_flatten(p);
    if (f.refused) return 1;
    for (const MegaTask &t : f.tasks) printf("%d %d %d %d %d %d %d %d\n", t.a.x, t.a.y, t.a.z, t.a.w, t.b.x, t.b.y, t.b.z, t.b.w);
    for (const Need2 &n : f.need) printf("%d %d\n", n.x, n.y);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "--dump")) return dump(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    // the synchronisation block: every hot word on a 128-byte line of its own, the version words right behind it
    static_assert(offsetof(MegaSync, status) == 4 && offsetof(MegaSync, pad) == 8, "status and the spare word keep their places");
    static_assert(offsetof(MegaSync, ghead) == 128 && offsetof(MegaSync, uhead) == 128 + 8 * 128, "queue heads on lines of their own");
    static_assert(offsetof(MegaSync, cukey) == 128 + 16 * 128 && offsetof(MegaSync, wflag) % 128 == 0, "W counters on lines of their own");
    static_assert(sizeof(MegaSync) == offsetof(MegaSync, wflag) + DGPAMD_MAXB * 128, "nothing behind the W counters");
    static_assert(sizeof(MegaTask) == 32 && sizeof(Task4) == 16 && sizeof(Need2) == 8, "eight ints per task, two per block");

    std::vector<int> nbks;
    for (int nbk = 1; nbk <= 33; ++nbk) nbks.push_back(nbk);
    nbks.push_back(48);
    nbks.push_back(79);
    const int batches[] = {1, 2, 3, 4, 5, 6, 8, 12, 16, DGPAMD_MAXB};
    // the default switches, and each override at its clamp ends (context.hip); lazy / slazy: 1 and the builder's cap (and past it)
    struct Set { const char *name; int64_t lazy, slazy, near, slag, look, queues; };
    const Set sets[] = {{"default", 0, 0, 3, 0, 1, 0},     {"lazy 1", 1, 1, 3, 0, 1, 0},          {"lazy 24", 24, 24, 3, 0, 1, 0},
                        {"lazy 1000", 1000, 1000, 3, 0, 1, 0}, {"near 0", 0, 0, 0, 0, 1, 0},       {"near 6", 0, 0, 6, 0, 1, 0},
                        {"slag 8", 0, 0, 3, 8, 1, 0},      {"look 0", 0, 0, 3, 0, 0, 0},          {"queues 1", 0, 0, 3, 0, 1, 1},
                        {"queues 2", 0, 0, 3, 0, 1, 2},    {"lazy 24 near 6 slag 8", 24, 24, 6, 8, 1, 0}, {"lazy 1 near 0", 1, 1, 0, 0, 1, 0},
                        {"lazy 1 near 0 look 0 queues 2", 1, 1, 0, 0, 0, 2}};
    for (int nbk : nbks)
        for (int inv = 0; inv < 2; ++inv) {
            where = "per-step tables, nbk " + std::to_string(nbk) + " inv " + std::to_string(inv);
            check_step_tables(nbk, inv != 0);
            for (const Set &s : sets)
                for (int batch : batches)
                    for (int dev = 0; dev < 2; ++dev) {   // an MI355X (256 CUs x 2 workgroups), and a device too small for two queues
                        Tuning tn = default_tuning();
                        tn.mega_lazy = s.lazy; tn.mega_slazy = s.slazy; tn.mega_near = s.near; tn.mega_slag = s.slag;
                        tn.mega_look = s.look; tn.mega_queues = s.queues;
                        where = std::string(s.name) + ", nbk " + std::to_string(nbk) + " inv " + std::to_string(inv) + " batch " +
                                std::to_string(batch) + (dev ? " on 16 CUs" : "");
                        check_plan(tn, nbk, inv != 0, batch, dev ? 16 : 256, 2, &s == &sets[0] && dev == 0);
                    }
        }
    // groups and critical workers: the overrides at their ends
    for (int batch : batches)
        for (int64_t groups : {1, 8})
            for (int64_t ncrit : {1, 1000}) {
                Tuning tn = default_tuning();
                tn.mega_groups = groups; tn.mega_ncrit = ncrit;
                where = "groups " + std::to_string(groups) + " ncrit " + std::to_string(ncrit) + " batch " + std::to_string(batch);
                check_plan(tn, 8, true, batch, 256, 2, false);
            }
    printf("two-queue guard: it counts with the device's %d workgroup slots and lets two queues through; by the launch's grid it would not at\n", 512);
    for (const auto &kv : premise) {
        printf("  inv, batch %s: nbk", kv.first.c_str());
        for (int nbk : kv.second) printf(" %d", nbk);
        printf("\n");
    }
    if (premise.empty()) printf("  no shape of the grid\n");
    printf(failures ? "potrf_table_check: %lld plans, %lld tables, %lld tasks walked, %d FAILED\n" : "potrf_table_check: %lld plans, %lld tables, %lld tasks walked, ok\n",
           plans, tables, tasks_walked, failures);
    return failures ? 1 : 0;
}
