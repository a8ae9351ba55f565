// The library's switches and the padding rule of its matrices: plain C++ with no HIP include, so that the host-only plan
// headers (potrf_plan.hpp) and the stand-alone checkers under tools/ see the same definitions as the kernels' files.
#pragma once
#include <stdint.h>

#define NB 64          // factorisation block / tile edge

// The DGPAMD_* switches of the C library as dgpamd_create found them (context.hip holds the one table: names, defaults, accepted
// values).  A context keeps the switches it was created under.  0 stands for "unset" where the default depends on the call.
struct Tuning {
    int64_t potrf_mode, fetch_spin, llik_args_copy;
    int64_t mega_lazy, mega_slazy, mega_near, mega_look, mega_slag, mega_queues, mega_ncrit, mega_split, mega_groups;
    int64_t jsep_tch, jsexp_tch, pair_chunk, sexp_form1, sexp_poly, jsep_pipe, jsep_log, jsep_noclass, jsep_diag;
    int64_t nn_filter, nn_store_once, vecchia_lds, poison_lds;
};

static inline int64_t padded_dim(int64_t n) { return ((n + 1 + NB - 1) / NB) * NB; }
