/* Stand-in for <gsl/gsl_linalg.h> (see gsl_math.h in this directory): the forward model uses nothing of it. */
#ifndef GSL_STANDIN_LINALG_H
#define GSL_STANDIN_LINALG_H
#include "gsl_blas.h"
#endif
