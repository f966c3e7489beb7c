// mi355q_gemm_v9f.hip -- the FULL-TILE launch of the 256 x 256 tile kernel (mi355q_gemm_v9_full.h says which launches those are):
// mi355q_gemm_v9.hip compiled as a translation unit of its own with V9_FULL_TU defined (see the note at the top of that file) -- one
// weight operand, one slice of K, every tile whole, no residual, no debug bits, all compile-time facts; plain kernel arguments; K-step 0
// requested in front of the side area's loads.  Same arithmetic, same order of summation, same stores: the general kernel's bits.
#define V9_FULL_TU 1
#include "mi355q_gemm_v9.hip"
