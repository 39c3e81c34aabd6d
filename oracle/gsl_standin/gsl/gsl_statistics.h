/* Stand-in for <gsl/gsl_statistics.h> (see gsl_math.h in this directory): the forward model uses nothing of it. */
#ifndef GSL_STANDIN_STATISTICS_H
#define GSL_STANDIN_STATISTICS_H
#endif
