// assoc_pheno.hip — the multi-phenotype kernels of pg_assoc_pheno_dev (shared decade scan + per-phenotype lambda search), c = 1..15
// (fifth translation unit of assoc.hip).
#define PG_ASSOC_PART 4
#include "assoc.hip"
