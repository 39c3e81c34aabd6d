/* Stand-in for <gsl/gsl_const_mksa.h> (see gsl_math.h in this directory): the two constants the forward model reads,
 * with the values GSL 2.5 publishes (CODATA 2006), as cited in oracle/oracle_constants.h. */
#ifndef GSL_STANDIN_CONST_MKSA_H
#define GSL_STANDIN_CONST_MKSA_H
#define GSL_CONST_MKSA_BOLTZMANN (1.3806504e-23)   /* kg m^2 / K s^2 */
#define GSL_CONST_MKSA_MOLAR_GAS (8.314472e0)      /* kg m^2 / K mol s^2 */
#endif
