// ainv.cpp -- host construction of the AINV and DIAG preconditioners (fp64).
//
// ainv_bridson restates cusp's nonsym_bridson_ainv as the reference calls it
// (MyAINV::Initilize, src/preconditioner.cu:140-201: drop tolerance .1, no bound
// on the entries per row, no linear dropping): the biconjugation of Benzi and
// Tuma with Bridson's right-looking updates.  With z_j, w_j = e_j at the start,
// for j = 0 .. n-1
//   u = A^T w_j,  l = A z_j,  p = w_j . l,  dinv[j] = 1 / p
//   z_i += (-u_i / p) z_j   for every i > j with u_i != 0, ascending
//   w_i += (-l_i / p) w_j   for every i > j with l_i != 0, ascending
// where a term of an update is dropped when |term| < tol.  (u and l are named
// by the matrix cusp hands its matrix_vector_product, A^T for u and A for l;
// that routine walks the rows the vector selects, b[col] += M[row][col] x[row].)
// The summation orders
// that fix the bits: u and l are accumulated over the vector's entries in
// ascending index and the matrix row's entries in stored order (the first
// product assigned, later ones added); p is an ascending merge from 0.
// M = Wt diag(dinv) Z approximates A^-1 (Z row i = z_i, Wt = the transpose of
// the matrix of rows w_i): Z unit lower, Wt unit upper triangular, ascending
// columns.
//
// Rows are flat sorted arrays (an update is a sorted merge), u and l dense
// accumulators with a touched list: the set-up is linear in the work the
// updates do, usable at a million rows.
//
// diag_nearest: MyDIAG::Initilize (src/preconditioner.cu:506-540).
#include <algorithm>
#include <cmath>
#include <utility>

#include "../gg_internal.h"

namespace gg {

namespace {

struct Ent {
    int c;
    double v;
};
using Row = std::vector<Ent>;

// stable transpose: column c's entries in ascending row order
Csr transpose(const Csr &A)
{
    Csr T;
    T.n = A.n;
    T.rp.assign(A.n + 1, 0);
    for (int k = 0; k < A.nnz(); k++) T.rp[A.ci[k] + 1]++;
    for (int c = 0; c < A.n; c++) T.rp[c + 1] += T.rp[c];
    T.ci.resize(A.nnz());
    T.v.resize(A.nnz());
    std::vector<int> pos(T.rp.begin(), T.rp.end() - 1);
    for (int r = 0; r < A.n; r++)
        for (int k = A.rp[r]; k < A.rp[r + 1]; k++) {
            const int o = pos[A.ci[k]]++;
            T.ci[o] = r;
            T.v[o] = A.v[k];
        }
    return T;
}

// sparse accumulator of one matrix-vector product (matrix_vector_product)
struct Acc {
    std::vector<double> val;
    std::vector<int> stamp, idx;
    explicit Acc(int n) : val(n, 0.0), stamp(n, -1) {}
    // b = M x: x's entries ascending, M's row entries in stored order
    void product(const Csr &M, const Row &x, int j)
    {
        idx.clear();
        for (const Ent &e : x)
            for (int k = M.rp[e.c]; k < M.rp[e.c + 1]; k++) {
                const int c = M.ci[k];
                const double prod = M.v[k] * e.v;
                if (stamp[c] != j) {
                    stamp[c] = j;
                    val[c] = prod;
                    idx.push_back(c);
                } else {
                    val[c] += prod;
                }
            }
    }
    bool has(int c, int j) const { return stamp[c] == j; }
};

// res += mult * op, a term dropped when |term| < tol (vector_add_inplace_drop
// with no bound on the row's entries); both rows ascending
void add_drop(Row &res, double mult, const Row &op, double tol, Row &tmp)
{
    tmp.clear();
    size_t a = 0;
    bool changed = false;
    for (const Ent &e : op) {
        const double term = mult * e.v;
        const double at = term < 0 ? -term : term;
        if (at < tol) continue;
        while (a < res.size() && res[a].c < e.c) tmp.push_back(res[a++]);
        if (a < res.size() && res[a].c == e.c) {
            tmp.push_back(Ent{e.c, res[a].v + term});
            a++;
        } else {
            tmp.push_back(Ent{e.c, term});
        }
        changed = true;
    }
    if (!changed) return;
    while (a < res.size()) tmp.push_back(res[a++]);
    res.assign(tmp.begin(), tmp.end());
}

}  // namespace

int ainv_bridson(const Csr &A, double tol, Csr &Z, Csr &Wt, std::vector<double> &dinv)
{
    if (!(tol >= 0.0)) return GG_EINVAL;   // negative or NaN
    const int n = A.n;
    const Csr At = transpose(A);
    std::vector<Row> z(n), w(n);
    for (int i = 0; i < n; i++) {
        z[i].push_back(Ent{i, 1.0});
        w[i].push_back(Ent{i, 1.0});
    }
    dinv.assign(n, 0.0);
    Acc u(n), l(n);
    std::vector<int> later;
    Row tmp;
    for (int j = 0; j < n; j++) {
        u.product(At, w[j], j);
        l.product(A, z[j], j);
        double p = 0.0;
        for (const Ent &e : w[j])
            if (l.has(e.c, j)) p += e.v * l.val[e.c];
        if (p == 0.0 || !std::isfinite(p)) return GG_EZEROPIVOT;
        dinv[j] = 1.0 / p;
        for (int pass = 0; pass < 2; pass++) {
            const Acc &s = pass == 0 ? u : l;
            std::vector<Row> &f = pass == 0 ? z : w;
            later.clear();
            for (int c : s.idx)
                if (c > j && s.val[c] != 0.0) later.push_back(c);
            std::sort(later.begin(), later.end());
            for (int i : later) add_drop(f[i], -s.val[i] / p, f[j], tol, tmp);
        }
    }
    // Z: row i = z_i
    Z = Csr{};
    Z.n = n;
    Z.rp.assign(n + 1, 0);
    long long tz = 0, tw = 0;
    for (int i = 0; i < n; i++) {
        tz += (long long)z[i].size();
        tw += (long long)w[i].size();
    }
    if (tz >= (1LL << 31) || tw >= (1LL << 31)) return GG_EINVAL;
    Z.ci.reserve(tz);
    Z.v.reserve(tz);
    for (int i = 0; i < n; i++) {
        for (const Ent &e : z[i]) {
            Z.ci.push_back(e.c);
            Z.v.push_back(e.v);
        }
        Z.rp[i + 1] = (int)Z.ci.size();
        Row().swap(z[i]);
    }
    // Wt: the transpose of the matrix whose row i is w_i
    Wt = Csr{};
    Wt.n = n;
    Wt.rp.assign(n + 1, 0);
    for (int i = 0; i < n; i++)
        for (const Ent &e : w[i]) Wt.rp[e.c + 1]++;
    for (int c = 0; c < n; c++) Wt.rp[c + 1] += Wt.rp[c];
    Wt.ci.resize(tw);
    Wt.v.resize(tw);
    std::vector<int> pos(Wt.rp.begin(), Wt.rp.end() - 1);
    for (int i = 0; i < n; i++)
        for (const Ent &e : w[i]) {
            const int o = pos[e.c]++;
            Wt.ci[o] = i;
            Wt.v[o] = e.v;
        }
    return GG_OK;
}

int diag_nearest(const Csr &A, std::vector<double> &inv)
{
    inv.assign(A.n, 0.0);
    for (int i = 0; i < A.n; i++) {
        double d = 0.0;
        long long dist = 2LL * A.n;
        for (int k = A.rp[i]; k < A.rp[i + 1]; k++) {
            const long long dd = std::llabs((long long)A.ci[k] - i);
            if (dd < dist) {       // strict: the first of two equally near entries wins
                dist = dd;
                d = A.v[k];
            }
        }
        if (d == 0.0) return GG_EZEROPIVOT;   // (an empty row leaves d = 0)
        inv[i] = 1.0 / d;
    }
    return GG_OK;
}

}  // namespace gg
