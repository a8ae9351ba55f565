// The register-resident Vecchia row kernels of the Matern-2.5 correlation (csrc/vecchia_row4.hpp).
#define VROW4_KIND DGPAMD_MATERN25
#include "vecchia_row4.hpp"
