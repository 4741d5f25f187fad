/* lapacke.h stand-in for building the reference's 2-D sources into oracle/_ref/libnlps_ref2d.so.
 *
 * Prototypes and renaming macros only: the six LAPACKE entry points the reference calls are mapped onto the
 * LAPACKE that scipy's bundled OpenBLAS exports under a scipy_ prefix (real LAPACK, the routines the reference
 * links).  The two Fortran symbols it also calls (dgetrf_, dgetri_) are renamed on the compiler command line
 * (oracle/orc.py::build_ref).  No arithmetic lives here. */
#ifndef NLPS_REF_SHIM_LAPACKE_H
#define NLPS_REF_SHIM_LAPACKE_H

#define LAPACK_ROW_MAJOR 101
#define LAPACK_COL_MAJOR 102

typedef int lapack_int;

lapack_int scipy_LAPACKE_dsyev(int layout, char jobz, char uplo, lapack_int n, double *a, lapack_int lda, double *w);
lapack_int scipy_LAPACKE_dgetrf(int layout, lapack_int m, lapack_int n, double *a, lapack_int lda, lapack_int *ipiv);
lapack_int scipy_LAPACKE_dgetri(int layout, lapack_int n, double *a, lapack_int lda, const lapack_int *ipiv);
lapack_int scipy_LAPACKE_dgetrs(int layout, char trans, lapack_int n, lapack_int nrhs, const double *a,
                                lapack_int lda, const lapack_int *ipiv, double *b, lapack_int ldb);
lapack_int scipy_LAPACKE_dgecon(int layout, char norm, lapack_int n, const double *a, lapack_int lda,
                                double anorm, double *rcond);
double scipy_LAPACKE_dlange(int layout, char norm, lapack_int m, lapack_int n, const double *a, lapack_int lda);

#define LAPACKE_dsyev scipy_LAPACKE_dsyev
#define LAPACKE_dgetrf scipy_LAPACKE_dgetrf
#define LAPACKE_dgetri scipy_LAPACKE_dgetri
#define LAPACKE_dgetrs scipy_LAPACKE_dgetrs
#define LAPACKE_dgecon scipy_LAPACKE_dgecon
#define LAPACKE_dlange scipy_LAPACKE_dlange

#endif
