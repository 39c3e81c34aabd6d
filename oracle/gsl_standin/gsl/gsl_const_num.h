/* Stand-in for <gsl/gsl_const_num.h> (see gsl_math.h in this directory): GSL 2.5's value (CODATA 1998). */
#ifndef GSL_STANDIN_CONST_NUM_H
#define GSL_STANDIN_CONST_NUM_H
#define GSL_CONST_NUM_AVOGADRO (6.02214199e23)     /* 1 / mol */
#endif
