// The two factorisation kernels, each in a file of its own, compiled as ONE unit in the order they had in chol.hip.  Compiled
// apart they come out of the same optimised IR with the same registers, LDS and instruction counts but in another instruction
// order (potrf_mega_kernel: 1064 of 14684 lines of its worker loop's set-up and register allocation; potrf_step_kernel: one
// instruction moved), and the one-launch fused inverse measured 1 % slower at two to ten matrices (profiles/chol_split.txt).
// Together they are the parent's code, instruction for instruction (tools/kernel_compare.py).
#include "potrf_step.hpp"
#include "potrf_mega.hpp"
