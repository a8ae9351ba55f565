// The register-resident Vecchia row kernels of the squared-exponential correlation (csrc/vecchia_row4.hpp).
#define VROW4_KIND DGPAMD_SEXP
#include "vecchia_row4.hpp"
