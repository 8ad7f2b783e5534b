// assoc_pheno_hi.hip — the multi-phenotype kernels of pg_assoc_pheno_dev, c = 16..PG_MAX_COVARIATES (sixth translation unit of assoc.hip).
#define PG_ASSOC_PART 5
#include "assoc.hip"
