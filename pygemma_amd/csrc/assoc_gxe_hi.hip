// assoc_gxe_hi.hip — GxE instantiations for shared c = 16..PG_MAX_COVARIATES - 1 (seventh translation unit of assoc.hip).
#define PG_ASSOC_PART 7
#include "assoc.hip"
