/*
 * ref_shim.cpp -- plain-array entry points to the reference's host routines.
 *
 * TEST INFRASTRUCTURE ONLY.  oracle/Makefile links this file with the
 * reference's src/SpMV_compute.cpp, src/iluk.cpp, src/itsol.cpp and
 * src/formatConvert.cpp (compiled from the reference checkout, never copied
 * here) and with the host GMRES engines slice_ref.py cuts out of src/gmres.cu
 * and src/preconditioner.cu (at the end of this file) into
 * _ref/libgg_ref.so; oracle/ref.py loads it.  Everything is built
 * with ref_widen.h in front, so the reference's `float` is double here and in
 * the declarations below.  No arithmetic happens in this file: it only moves
 * arrays into and out of the reference's own structures.
 */
#include "SpMV.h"
#include "gpuData.h"

/* defined in src/iluk.cpp, declared in no header */
int setupILU(iluptr lu, int n);
int lofC(int lofM, csptr csmat, iluptr lu, FILE *fp);
/* defined in src/formatConvert.cpp, declared in no header */
void sortDouble(int *col_idx, double *a, int start, int end);
void LDcsc2csr(long nnz, long m, long n, long *p, long *i, double *x, int **out_rp, int **out_ci,
               float **out_v);

namespace {

struct Factor {
    int n;
    int ierr;
    int numeric;
    csptr A;
    iluptr lu;
};

/* CSR arrays -> the SparMat ilukC reads, rows in the given order */
csptr make_cs(int n, const int *rp, const int *ci, const double *v)
{
    csptr A = (csptr)malloc(sizeof(SparMat));
    setupCS(A, n, 1);
    for (int i = 0; i < n; i++) {
        int len = rp[i + 1] - rp[i];
        A->nzcount[i] = len;
        A->ja[i] = NULL;
        A->ma[i] = NULL;
        if (len <= 0) continue;
        A->ja[i] = (int *)malloc(sizeof(int) * len);
        A->ma[i] = (float *)malloc(sizeof(float) * len);
        for (int j = 0; j < len; j++) {
            A->ja[i][j] = ci[rp[i] + j];
            A->ma[i][j] = v[rp[i] + j];
        }
    }
    return A;
}

}  // namespace

extern "C" {

int ref_sizeof_real(void) { return (int)sizeof(float); }

void ref_spmv(int n, const int *rp, const int *ci, const double *v, const double *x, double *y)
{
    computeSpMV(y, v, rp, ci, x, n);
}

/* x must come in zeroed: the forward loop divides it before it is assigned */
void ref_lusolve(int n, const int *l_rp, const int *l_ci, const double *l_v,
                 const int *u_rp, const int *u_ci, const double *u_v,
                 const double *y, double *x)
{
    LUSolve_ignoreZero(x, l_v, l_rp, l_ci, u_v, u_rp, u_ci, y, n);
}

/* numeric = 0: setupILU + lofC (pattern only); 1: ilukC.  *status = the
 * routine's return value; the handle holds what it left behind. */
void *ref_iluk(int numeric, int lofM, int n, const int *rp, const int *ci, const double *v,
               int *status)
{
    Factor *f = (Factor *)malloc(sizeof(Factor));
    FILE *log = fopen("/dev/null", "w");
    f->n = n;
    f->numeric = numeric;
    f->A = make_cs(n, rp, ci, v);
    f->lu = (iluptr)malloc(sizeof(ILUSpar));
    if (numeric) {
        f->ierr = ilukC(lofM, f->A, f->lu, log ? log : stderr);
    } else {
        setupILU(f->lu, n);
        f->ierr = lofC(lofM, f->A, f->lu, log ? log : stderr);
    }
    if (log) fclose(log);
    *status = f->ierr;
    return f;
}

/* row lengths of L and U (n each); only after status 0 */
void ref_iluk_counts(void *h, int *lnz, int *unz)
{
    Factor *f = (Factor *)h;
    for (int i = 0; i < f->n; i++) {
        lnz[i] = f->lu->L->nzcount[i];
        unz[i] = f->lu->U->nzcount[i];
    }
}

/* rows concatenated in the order the reference left them; l_v, d, u_v may be
 * NULL (and must be after the pattern-only call) */
void ref_iluk_get(void *h, int *l_ci, double *l_v, double *d, int *u_ci, double *u_v)
{
    Factor *f = (Factor *)h;
    int pl = 0, pu = 0;
    for (int i = 0; i < f->n; i++) {
        for (int j = 0; j < f->lu->L->nzcount[i]; j++, pl++) {
            l_ci[pl] = f->lu->L->ja[i][j];
            if (l_v) l_v[pl] = f->lu->L->ma[i][j];
        }
        for (int j = 0; j < f->lu->U->nzcount[i]; j++, pu++) {
            u_ci[pu] = f->lu->U->ja[i][j];
            if (u_v) u_v[pu] = f->lu->U->ma[i][j];
        }
        if (d) d[i] = f->lu->D[i];
    }
}

/* the handle's rows are left to the process (a failed or pattern-only
 * factorization leaves row pointers unset, so the reference's cleanILU cannot
 * be used on it) */
void ref_iluk_free(void *h) { free(h); }

void ref_coo2csr_double(int n, int nz, double *a, int *i_idx, int *j_idx)
{
    coo2csrDouble_in(n, nz, a, i_idx, j_idx);
}

void ref_sort_double(int *col_idx, double *a, int start, int end)
{
    ::sortDouble(col_idx, a, start, end);
}

/* out_rp: max(nnz, m + 1) ints; out_ci, out_v: nnz */
void ref_ldcsc2csr(long nnz, long m, long n, long *p, long *i, double *x,
                   int *out_rp, int *out_ci, double *out_v)
{
    int *rp = NULL, *ci = NULL;
    float *v = NULL;
    LDcsc2csr(nnz, m, n, p, i, x, &rp, &ci, &v);
    long cap = nnz > m + 1 ? nnz : m + 1;
    memcpy(out_rp, rp, sizeof(int) * cap);
    memcpy(out_ci, ci, sizeof(int) * nnz);
    for (long k = 0; k < nnz; k++) out_v[k] = v[k];
    free(rp); free(ci); free(v);
}

void ref_ldcsc2csr_double(long nzmax, long m, long n, long *p, long *i, double *x,
                          int *out_rp, int *out_ci, double *out_v)
{
    ucr_cs_dl M;
    M.shallowCpy(nzmax, m, n, p, i, x, -1);
    MySpMatrixDouble D;
    LDcsc2csrMySpMatrixDouble(&D, &M);
    long cap = nzmax > m + 1 ? nzmax : m + 1;
    memcpy(out_rp, D.rowIndices, sizeof(int) * cap);
    memcpy(out_ci, D.indices, sizeof(int) * nzmax);
    memcpy(out_v, D.val, sizeof(double) * nzmax);
    free(D.rowIndices); free(D.indices); free(D.val);
}

}  // extern "C"

#ifdef GG_REF_ENGINES
/*
 * The reference's host GMRES engines.  src/gmres.cu and src/preconditioner.cu
 * need cusp, cublas and <<<>>> and do not compile as files; slice_ref.py cuts
 * the plain C++ functions out of them into _ref/gmres_host_slice.cpp (the
 * vector helpers, Update, the two plane-rotation routines, GMRES_leftILU0, the
 * unpreconditioned GMRES, GMRESilu and MyILUPP::HostPrecond_rhs /
 * _starting_value / _left / _right), which is included below.  GMRESilu takes
 * a Preconditioner &: this project's compat header has the reference's layout.
 * MyILUPP is declared here with exactly the members the four routines read;
 * the reference's own class drags in cusparse.
 */
#include "../include/compat/preconditioner.h"

class MyILUPP : public Preconditioner {
public:
    IndexType *l_rowIndices, *l_indices;
    IndexType *u_rowIndices, *u_indices;
    double *l_val_double, *u_val_double;
    ValueType *middle_val;
    IndexType *permRow_indices, *permCol_indices;
    double *lscale_val, *rscale_val;
    float *tmpvector;

    /* never reached by GMRESilu */
    void HostPrecond(const ValueType *, ValueType *) { abort(); }
    void DevPrecond(const ValueType *, ValueType *) { abort(); }
    void Initilize(const MySpMatrix &) { abort(); }
    void DevPrecond_rhs(float *, float *) { abort(); }
    void DevPrecond_right(float *, float *) { abort(); }
    void DevPrecond_left(float *, float *) { abort(); }
    void DevPrecond_starting_value(float *, float *) { abort(); }

    /* defined by the slice */
    void HostPrecond_rhs(const ValueType *i_data, ValueType *o_data);
    void HostPrecond_right(const ValueType *i_data, ValueType *o_data);
    void HostPrecond_left(const ValueType *i_data, ValueType *o_data);
    void HostPrecond_starting_value(const ValueType *i_data, ValueType *o_data);
};

#include "_ref/gmres_host_slice.cpp"

namespace {
/* GMRES_leftILU0 and GMRES write a line to cout per iteration */
struct QuietCout {
    std::streambuf *old;
    QuietCout() : old(std::cout.rdbuf(NULL)) {}
    ~QuietCout() { std::cout.rdbuf(old); }
};

void fill_ilupp(MyILUPP &P, int n, int *l_rp, int *l_ci, double *l_v, int *u_rp, int *u_ci, double *u_v,
                double *middle, int *perm_row, int *perm_col, double *lscale, double *rscale)
{
    P.numRows = n;
    P.l_rowIndices = l_rp; P.l_indices = l_ci; P.l_val_double = l_v;
    P.u_rowIndices = u_rp; P.u_indices = u_ci; P.u_val_double = u_v;
    P.middle_val = middle;
    P.permRow_indices = perm_row; P.permCol_indices = perm_col;
    P.lscale_val = lscale; P.rscale_val = rscale;
    P.tmpvector = (float *)malloc(sizeof(float) * (n > 0 ? n : 1));
}
}  // namespace

extern "C" {

int ref_has_engines(void) { return 1; }

/* Each engine returns its ret and leaves x, *max_iter and *tol as it left them. */
int ref_gmres_left_ilu0(int n, const int *rp, const int *ci, const double *v,
                        const int *l_rp, const int *l_ci, const double *l_v,
                        const int *u_rp, const int *u_ci, const double *u_v,
                        const double *b, double *x, int m, int *max_iter, double *tol)
{
    QuietCout q;
    return GMRES_leftILU0(v, rp, ci, x, b, n, m, max_iter, tol, l_v, l_rp, l_ci, u_v, u_rp, u_ci);
}

int ref_gmres_plain(int n, const int *rp, const int *ci, const double *v,
                    const double *b, double *x, int m, int *max_iter, double *tol)
{
    QuietCout q;
    return GMRES(v, rp, ci, x, b, n, m, max_iter, tol);
}

int ref_gmres_split(int n, const int *rp, const int *ci, const double *v,
                    int *l_rp, int *l_ci, double *l_v, int *u_rp, int *u_ci, double *u_v,
                    double *middle, int *perm_row, int *perm_col, double *lscale, double *rscale,
                    const double *b, double *x, int m, int *max_iter, double *tol)
{
    QuietCout q;
    MyILUPP P;
    fill_ilupp(P, n, l_rp, l_ci, l_v, u_rp, u_ci, u_v, middle, perm_row, perm_col, lscale, rscale);
    int ret = GMRESilu(v, rp, ci, x, b, n, m, max_iter, tol, P);
    free(P.tmpvector);
    return ret;
}

/* one of MyILUPP's four host maps on its own: which = 0 HostPrecond_left,
 * 1 _right, 2 _starting_value, 3 _rhs */
void ref_split_apply(int which, int n,
                     int *l_rp, int *l_ci, double *l_v, int *u_rp, int *u_ci, double *u_v,
                     double *middle, int *perm_row, int *perm_col, double *lscale, double *rscale,
                     const double *in, double *out)
{
    MyILUPP P;
    fill_ilupp(P, n, l_rp, l_ci, l_v, u_rp, u_ci, u_v, middle, perm_row, perm_col, lscale, rscale);
    if (which == 0) P.HostPrecond_left(in, out);
    else if (which == 1) P.HostPrecond_right(in, out);
    else if (which == 2) P.HostPrecond_starting_value(in, out);
    else P.HostPrecond_rhs(in, out);
    free(P.tmpvector);
}

}  // extern "C"
#endif /* GG_REF_ENGINES */
