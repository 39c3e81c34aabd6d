/* Stand-in for <gsl/gsl_blas.h> (see gsl_math.h in this directory): gsl_vector and gsl_matrix with GSL's field order
 * (size, stride, data, block, owner / size1, size2, tda, data, block, owner), so that a matrix built by a caller who
 * mirrors GSL's layout is read correctly, and the handful of accessors kernel() and its helpers call. */
#ifndef GSL_STANDIN_BLAS_H
#define GSL_STANDIN_BLAS_H
#include <stdlib.h>
#include <string.h>

typedef struct { size_t size; double *data; } gsl_block;
typedef struct { size_t size, stride; double *data; gsl_block *block; int owner; } gsl_vector;
typedef struct { size_t size1, size2, tda; double *data; gsl_block *block; int owner; } gsl_matrix;

static inline gsl_vector *gsl_vector_alloc(size_t n) {
	gsl_vector *v = (gsl_vector *) malloc(sizeof(gsl_vector));
	v->size = n; v->stride = 1; v->block = NULL; v->owner = 1;
	v->data = (double *) calloc(n ? n : 1, sizeof(double));
	return v;
}
static inline void gsl_vector_free(gsl_vector *v) { if(v) { if(v->owner) free(v->data); free(v); } }
static inline double gsl_vector_get(const gsl_vector *v, size_t i) { return v->data[i*v->stride]; }
static inline void gsl_vector_set(gsl_vector *v, size_t i, double x) { v->data[i*v->stride] = x; }
static inline int gsl_vector_memcpy(gsl_vector *dest, const gsl_vector *src) {
	for(size_t i = 0; i < src->size; i++) dest->data[i*dest->stride] = src->data[i*src->stride];
	return 0;
}
static inline double gsl_matrix_get(const gsl_matrix *m, size_t i, size_t j) { return m->data[i*m->tda + j]; }
static inline void gsl_matrix_set(gsl_matrix *m, size_t i, size_t j, double x) { m->data[i*m->tda + j] = x; }
static inline void gsl_matrix_set_zero(gsl_matrix *m) {
	for(size_t i = 0; i < m->size1; i++) memset(m->data + i*m->tda, 0, m->size2*sizeof(double));
}

#endif
