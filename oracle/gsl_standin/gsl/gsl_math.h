/* Stand-in for <gsl/gsl_math.h>, written for this project: NOT part of GSL and not copied from it.
 *
 * oracle/Makefile's `ref` target compiles the reference's CPU forward model (src/jurassic.c, src/CPUdrivers.c) where
 * the reference tree lies; its jurassic.h:42-47 includes six GSL headers, and GSL is not installed.  The six files in
 * this directory hold only what those two sources use: gsl_finite, gsl_log1p, gsl_expm1, gsl_pow_2/3, GSL_MAX/MIN,
 * GSL_NAN, three physical constants, and get/set/alloc of gsl_vector / gsl_matrix.
 *
 * gsl_expm1 and gsl_log1p are libm's expm1 and log1p here.  GSL 2.5 has implementations of its own (sys/expm1.c,
 * sys/log1p.c), so planck() and brightness() of the library built with these headers are "the reference's source with
 * libm", not a GSL build; they may differ from a GSL build in the last bits.
 */
#ifndef GSL_STANDIN_MATH_H
#define GSL_STANDIN_MATH_H
#include <math.h>

#define GSL_NAN (NAN)
#define GSL_MAX(a, b) ((a) > (b) ? (a) : (b))
#define GSL_MIN(a, b) ((a) < (b) ? (a) : (b))
#define GSL_MAX_DBL(a, b) GSL_MAX(a, b)
#define GSL_MIN_DBL(a, b) GSL_MIN(a, b)

static inline int gsl_finite(double x) { return isfinite(x) ? 1 : 0; }
static inline double gsl_log1p(double x) { return log1p(x); }
static inline double gsl_expm1(double x) { return expm1(x); }
static inline double gsl_pow_2(double x) { return x*x; }
static inline double gsl_pow_3(double x) { return x*x*x; }

#endif
