// assoc_gxe.hip — the GxE kernels of pg_assoc_gxe_dev (x among the covariates, x o e tested), shared c = 1..15, and
// pg_gxe_scale_u_dev (sixth translation unit of assoc.hip).
#define PG_ASSOC_PART 6
#include "assoc.hip"
