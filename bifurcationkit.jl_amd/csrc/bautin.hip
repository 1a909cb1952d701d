// Bautin (generalised Hopf) normal form, matrix-free: bautin_normal_form (src/codim2/NormalForms.jl:642-829, detailed = false)
// for BK_PDE_CGL2D.  At a Hopf point (x, p, omega) with q = zeta, p0 = zeta*, <zeta, zeta*> = 1, dot(p0, h) = sum conj(p0) h and
// B, C, D, E the 2nd .. 5th derivatives of the cGL right-hand side at x (pointwise; hopf_pw.h), after Kuznetsov (1999), section 7:
//
//   H20 = (2 i omega - J) \ B(q, q) = 2 Psi200,   H11 = -J \ B(q, conj q) = Psi110         (bk_hopf_normal_form has both)
//   G21 = dot(p0, C(q, q, conj q) + B(conj q, H20) + 2 B(q, H11)) = 2 conj(b)               (b = <bv, zeta*> conjugates bv)
//   H30 = (3 i omega - J) \ (C(q, q, q) + 3 B(q, H20))                                        bk_gmres_cshift
//   H21 : [J - i omega, q; p0^H, 0][H21; s] = [G21 q - (C(q, q, conj q) + B(conj q, H20) + 2 B(q, H11)); 0]   bk_bls_bordering_cshift
//   H31 = (2 i omega - J) \ (D(q, q, q, conj q) + 3 C(q, q, H11) + 3 C(q, conj q, H20) + 3 B(H20, H11) + B(conj q, H30)
//                            + 3 B(q, H21) - 3 G21 H20)                                       bk_gmres_cshift
//   H22 = -J \ (D(q, q, conj q, conj q) + 4 C(q, conj q, H11) + 2 Re C(conj q, conj q, H20) + 2 B(H11, H11)
//               + 4 Re B(conj q, H21) + B(conj H20, H20) - 4 Re(G21) H11)                     real solve
//   G32 = dot(p0, E(q, q, q, conj q, conj q) + D(q, q, q, conj H20) + 3 D(q, conj q, conj q, H20) + 6 D(q, q, conj q, H11)
//                 + C(conj q, conj q, H30) + 3 C(q, q, conj H21) + 6 C(q, conj q, H21) + 3 C(q, conj H20, H20) + 6 C(q, H11, H11)
//                 + 6 C(conj q, H20, H11) + 2 B(conj q, H31) + 3 B(q, H22) + B(conj H20, H30) + 3 B(conj H21, H20) + 6 B(H11, H21))
//   l2 = Re G32 / 12
//
// D and E are analytic (only the quintic term contributes) where the reference nests central differences of d3F (:757-794).  The
// right-hand sides of the four solves come from two writing passes and G32 from one reducing pass over fifteen vectors; every
// tensor is contracted with q once per point and field and the partial contractions are shared between the terms.  Complex
// vectors are (re, im) pairs of real device vectors of the two stacked fields.
#include <cmath>

#include "common.h"
#include "hopf_pw.h"
#include "minaug.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

// ------------------------------------------------------------------ passes
// the tensors of field f out of the stacked arrays of cgl_hess / cgl_d3 / cgl_d4 / cgl_d5
template <int K>
__device__ __forceinline__ void field_of(const double* all, int f, double (&t)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = all[K * f + j];
}

// component f of a 2-vector
__device__ __forceinline__ Cx at(Cx2 v, int f) { return f ? v.b : v.a; }
__device__ __forceinline__ double at(Re2 v, int f) { return f ? v.b : v.a; }

// One pass over u, q, H20, H11 that writes the right-hand sides of the H30 and H21 solves:
//   h30 = C(q, q, q) + 3 B(q, H20),     h21 = G21 q - ((C(q, q, conj q) + B(conj q, H20)) + 2 B(q, H11))
// 6 read and 4 write streams.
struct BautinRhs3 {
    static constexpr int NIN = 12, NOUT = 8, U = 1, FIELDS = 2;
    static constexpr bool JOINT = true;
    const double* in[NIN / FIELDS];     // u, qr, qi, H20r, H20i, H11
    double* out[NOUT / FIELDS];         // h30r, h30i, h21r, h21i
    CglCoef c;
    double g21r, g21i;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&o)[NOUT]) const {
        const double u1 = x[0], u2 = x[1];
        const Cx2 q{{x[2], x[4]}, {x[3], x[5]}}, A{{x[6], x[8]}, {x[7], x[9]}}, qc = conj(q);
        const Re2 B{x[10], x[11]};
        const Cx G21{g21r, g21i};
        double h[6], t[8];
        cgl_hess(c, u1, u2, h);
        cgl_d3(c, u1, u2, t);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            double Hf[3], Tf[4];
            field_of<3>(h, f, Hf);
            field_of<4>(t, f, Tf);
            Cx Hq[2], Hqc[2], Tq[3], Tqq[2];
            sym_lower<2>(Hf, q, Hq);
            sym_conj<2>(Hq, Hqc);
            sym_lower<3>(Tf, q, Tq);
            sym_lower<2>(Tq, q, Tqq);
            const Cx h30 = sym_dot(Tqq, q) + 3.0 * sym_dot(Hq, A);
            const Cx v21 = (sym_dot(Tqq, qc) + sym_dot(Hqc, A)) + 2.0 * sym_dot(Hq, B);
            const Cx h21 = G21 * at(q, f) - v21;
            o[f] = h30.r;
            o[2 + f] = h30.i;
            o[4 + f] = h21.r;
            o[6 + f] = h21.i;
        }
    }
};

// One pass over u, q, H20, H11, H30, H21 that writes the right-hand sides of the H31 and H22 solves:
//   h31 = (D(q, q, q, conj q) + B(conj q, H30)) + 3 ((((C(q, q, H11) + C(q, conj q, H20)) + B(H11, H20)) + B(q, H21)) - G21 H20)
//   h22 = ((Re D(q, q, conj q, conj q) + Re B(H20, conj H20)) + 2 (Re C(conj q, conj q, H20) + B(H11, H11)))
//         + 4 ((Re C(q, conj q, H11) + Re B(conj q, H21)) - Re(G21) H11)
// 10 read and 3 write streams.
struct BautinRhs4 {
    static constexpr int NIN = 20, NOUT = 6, U = 1, FIELDS = 2;
    static constexpr bool JOINT = true;
    const double* in[NIN / FIELDS];     // u, qr, qi, H20r, H20i, H11, H30r, H30i, H21r, H21i
    double* out[NOUT / FIELDS];         // h31r, h31i, h22
    CglCoef c;
    double g21r, g21i;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&o)[NOUT]) const {
        const double u1 = x[0], u2 = x[1];
        const Cx2 q{{x[2], x[4]}, {x[3], x[5]}}, A{{x[6], x[8]}, {x[7], x[9]}}, qc = conj(q);
        const Re2 B{x[10], x[11]};
        const Cx2 H30{{x[12], x[14]}, {x[13], x[15]}}, H21{{x[16], x[18]}, {x[17], x[19]}};
        const Cx G21{g21r, g21i};
        double h[6], t[8], d[10];
        cgl_hess(c, u1, u2, h);
        cgl_d3(c, u1, u2, t);
        cgl_d4(c, u1, u2, d);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            double Hf[3], Tf[4], Df[5], HB[2];
            field_of<3>(h, f, Hf);
            field_of<4>(t, f, Tf);
            field_of<5>(d, f, Df);
            Cx Hq[2], Hqc[2], HA[2], Tq[3], Tqq[2], Tqqc[2], Tqb[2], Dq[4], Dqq[3], Dqqq[2], Dqqb[2];
            sym_lower<2>(Hf, q, Hq);
            sym_conj<2>(Hq, Hqc);
            sym_lower<2>(Hf, A, HA);
            sym_lower<2>(Hf, B, HB);
            sym_lower<3>(Tf, q, Tq);
            sym_lower<2>(Tq, q, Tqq);
            sym_conj<2>(Tqq, Tqqc);
            sym_lower<2>(Tq, qc, Tqb);
            sym_lower<4>(Df, q, Dq);
            sym_lower<3>(Dq, q, Dqq);
            sym_lower<2>(Dqq, q, Dqqq);
            sym_lower<2>(Dqq, qc, Dqqb);
            const Cx t3 = (((sym_dot(Tqq, B) + sym_dot(Tqb, A)) + sym_dot(HB, A)) + sym_dot(Hq, H21)) - G21 * at(A, f);
            const Cx h31 = (sym_dot(Dqqq, qc) + sym_dot(Hqc, H30)) + 3.0 * t3;
            const double r0 = sym_dot(Dqqb, qc).r + sym_dot(HA, conj(A)).r;
            const double r2 = sym_dot(Tqqc, A).r + sym_dot(HB, B);
            const double r4 = (sym_dot(Tqb, B).r + sym_dot(Hqc, H21).r) - g21r * at(B, f);
            o[f] = h31.r;
            o[2 + f] = h31.i;
            o[4 + f] = (r0 + 2.0 * r2) + 4.0 * r4;
        }
    }
};

// One pass over u, q, p0, H20, H11, H30, H21, H31, H22: two partial sums per workgroup, (Re G32, Im G32).  Per point and field f
// the fifteen terms are grouped by their last argument,
//   v_f = E(q, q, q, conj q, conj q)
//       + D(q, q, q, .) conj H20 + D(q, q, conj q, .) 6 H11 + conj(D(q, q, conj q, .)) 3 H20
//       + conj(C(q, q, .)) H30 + C(q, q, .) 3 conj H21 + C(q, conj q, .) 6 H21 + C(q, ., .) : W + conj(C(q, ., .)) : 6 (H20, H11)
//       + conj(B(q, .)) 2 H31 + B(q, .) 3 H22 + B(H30, .) conj H20 + B(H20, .) 3 conj H21 + B(H11, .) 6 H21
// with the real symmetric weights W = 3 Re(conj H20 H20') + 6 H11 H11', and G32 += conj(p0_f) v_f is formed once per point.
struct BautinContract {
    static constexpr int NIN = 30, NV = 2, U = 1, FIELDS = 2;
    const double* in[NIN / FIELDS];     // u, qr, qi, pr, pi, H20r, H20i, H11, H30r, H30i, H21r, H21i, H31r, H31i, H22
    CglCoef c;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double u1 = x[0], u2 = x[1];
        const Cx2 q{{x[2], x[4]}, {x[3], x[5]}}, p0{{x[6], x[8]}, {x[7], x[9]}}, A{{x[10], x[12]}, {x[11], x[13]}}, qc = conj(q),
            Ac = conj(A);
        const Re2 B{x[14], x[15]};
        const Cx2 H30{{x[16], x[18]}, {x[17], x[19]}}, H21{{x[20], x[22]}, {x[21], x[23]}}, H31{{x[24], x[26]}, {x[25], x[27]}},
            H21c = conj(H21);
        const Re2 H22{x[28], x[29]};
        double h[6], t[8], d[10], e[12];
        cgl_hess(c, u1, u2, h);
        cgl_d3(c, u1, u2, t);
        cgl_d4(c, u1, u2, d);
        cgl_d5(c, e);
        // W = 3 Re(conj H20 H20') + 6 H11 H11'
        const double W11 = 3.0 * (A.a.r * A.a.r + A.a.i * A.a.i) + 6.0 * (B.a * B.a);
        const double W12 = 3.0 * (A.a.r * A.b.r + A.a.i * A.b.i) + 6.0 * (B.a * B.b);
        const double W22 = 3.0 * (A.b.r * A.b.r + A.b.i * A.b.i) + 6.0 * (B.b * B.b);
        Cx g{0.0, 0.0};
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            double Hf[3], Tf[4], Df[5], Ef[6], HB[2];
            field_of<3>(h, f, Hf);
            field_of<4>(t, f, Tf);
            field_of<5>(d, f, Df);
            field_of<6>(e, f, Ef);
            Cx Hq[2], Hqc[2], HA[2], HC[2], Tq[3], Tqc[3], Tqq[2], Tqqc[2], Tqb[2], Dq[4], Dqq[3], Dqqq[2], Dqqb[2], Dqqbc[2], Eq[5],
                Eqq[4], Eqqq[3], Eqqqb[2];
            sym_lower<2>(Hf, q, Hq);
            sym_conj<2>(Hq, Hqc);
            sym_lower<2>(Hf, A, HA);
            sym_lower<2>(Hf, B, HB);
            sym_lower<2>(Hf, H30, HC);
            sym_lower<3>(Tf, q, Tq);
            sym_conj<3>(Tq, Tqc);
            sym_lower<2>(Tq, q, Tqq);
            sym_conj<2>(Tqq, Tqqc);
            sym_lower<2>(Tq, qc, Tqb);
            sym_lower<4>(Df, q, Dq);
            sym_lower<3>(Dq, q, Dqq);
            sym_lower<2>(Dqq, q, Dqqq);
            sym_lower<2>(Dqq, qc, Dqqb);
            sym_conj<2>(Dqqb, Dqqbc);
            sym_lower<5>(Ef, q, Eq);
            sym_lower<4>(Eq, q, Eqq);
            sym_lower<3>(Eqq, q, Eqqq);
            sym_lower<2>(Eqqq, qc, Eqqqb);
            const Cx v5 = sym_dot(Eqqqb, qc);
            const Cx v4 = (sym_dot(Dqqq, Ac) + 3.0 * sym_dot(Dqqbc, A)) + 6.0 * sym_dot(Dqqb, B);
            const Cx v3a = (sym_dot(Tqqc, H30) + 3.0 * sym_dot(Tqq, H21c)) + 6.0 * sym_dot(Tqb, H21);
            const Cx v3b = ((W11 * Tq[0] + (2.0 * W12) * Tq[1]) + W22 * Tq[2]) + 6.0 * sym_dot(Tqc, A, Cx2{cx(B.a), cx(B.b)});
            const Cx v2a = 2.0 * sym_dot(Hqc, H31) + 3.0 * sym_dot(Hq, H22);
            const Cx v2b = (sym_dot(HC, Ac) + 3.0 * sym_dot(HA, H21c)) + 6.0 * sym_dot(HB, H21);
            const Cx v = ((v5 + v4) + (v3a + v3b)) + (v2a + v2b);
            g = g + conj(at(p0, f)) * v;
        }
        s[0] += g.r;
        s[1] += g.i;
    }
};

// ------------------------------------------------------------------ launchers; n = 2 N, the local length of both fields
int v_bautin_rhs3(bk_ctx* ctx, size_t n, const CglCoef& c, const double* const (&S)[6], const double g21[2], double* const (&O)[4]) {
    BautinRhs3 pass{{}, {}, c, g21[0], g21[1]};
    for (int k = 0; k < 6; ++k) pass.in[k] = S[k];
    for (int k = 0; k < 4; ++k) pass.out[k] = O[k];
    return stream_write(ctx, "bautin_rhs3", n / 2, pass);
}

int v_bautin_rhs4(bk_ctx* ctx, size_t n, const CglCoef& c, const double* const (&S)[10], const double g21[2], double* const (&O)[3]) {
    BautinRhs4 pass{{}, {}, c, g21[0], g21[1]};
    for (int k = 0; k < 10; ++k) pass.in[k] = S[k];
    for (int k = 0; k < 3; ++k) pass.out[k] = O[k];
    return stream_write(ctx, "bautin_rhs4", n / 2, pass);
}

// out[2] = (Re G32, Im G32)
int v_bautin_contract(bk_ctx* ctx, size_t n, const CglCoef& c, const double* const (&S)[15], double* out) {
    BautinContract pass{{}, c};
    for (int k = 0; k < 15; ++k) pass.in[k] = S[k];
    return stream_reduce(ctx, "bautin_contract", n / 2, pass, out);
}

// every output distinct from every input and from the other outputs
template <int NI, int NO>
int check_alias(bk_ctx* ctx, const char* what, const double* const (&ins)[NI], double* const (&outs)[NO]) {
    for (int k = 0; k < NO; ++k) {
        for (const double* i : ins)
            if (outs[k] == i) return set_error(ctx, "%s: an output aliases an input", what);
        for (int j = 0; j < k; ++j)
            if (outs[k] == outs[j]) return set_error(ctx, "%s: the output vectors must be distinct", what);
    }
    return 0;
}

template <int N>
bool any_null(const double* const (&p)[N]) {
    for (const double* v : p)
        if (!v) return true;
    return false;
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_bautin_rhs3(bk_problem* prob, const double* u, const double* params, int nparams, const double* q_re, const double* q_im,
                   const double* h20_re, const double* h20_im, const double* h11, const double g21[2], double* h30_re,
                   double* h30_im, double* h21_re, double* h21_im) {
    const double* const S[6] = {u, q_re, q_im, h20_re, h20_im, h11};
    double* const O[4] = {h30_re, h30_im, h21_re, h21_im};
    const double* const Oc[4] = {h30_re, h30_im, h21_re, h21_im};
    if (!prob || !params || !g21 || any_null(S) || any_null(Oc)) return -1;
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, 0, &c));
    BK_TRY(check_alias(prob->ctx, "bk_bautin_rhs3", S, O));
    return v_bautin_rhs3(prob->ctx, prob->nloc, c, S, g21, O);
}

int bk_bautin_rhs4(bk_problem* prob, const double* u, const double* params, int nparams, const double* q_re, const double* q_im,
                   const double* h20_re, const double* h20_im, const double* h11, const double* h30_re, const double* h30_im,
                   const double* h21_re, const double* h21_im, const double g21[2], double* h31_re, double* h31_im, double* h22) {
    const double* const S[10] = {u, q_re, q_im, h20_re, h20_im, h11, h30_re, h30_im, h21_re, h21_im};
    double* const O[3] = {h31_re, h31_im, h22};
    const double* const Oc[3] = {h31_re, h31_im, h22};
    if (!prob || !params || !g21 || any_null(S) || any_null(Oc)) return -1;
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, 0, &c));
    BK_TRY(check_alias(prob->ctx, "bk_bautin_rhs4", S, O));
    return v_bautin_rhs4(prob->ctx, prob->nloc, c, S, g21, O);
}

int bk_bautin_contract(bk_problem* prob, const double* u, const double* params, int nparams, const double* q_re, const double* q_im,
                       const double* p_re, const double* p_im, const double* h20_re, const double* h20_im, const double* h11,
                       const double* h30_re, const double* h30_im, const double* h21_re, const double* h21_im,
                       const double* h31_re, const double* h31_im, const double* h22, double out[2]) {
    const double* const S[15] = {u, q_re, q_im, p_re, p_im, h20_re, h20_im, h11, h30_re, h30_im, h21_re, h21_im, h31_re, h31_im, h22};
    if (!prob || !params || !out || any_null(S)) return -1;
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, 0, &c));
    return v_bautin_contract(prob->ctx, prob->nloc, c, S, out);
}

int bk_bautin_normal_form(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, double omega,
                          const double* z_re, const double* z_im, const double* zs_re, const double* zs_im, const double* psi110,
                          const double* psi200_re, const double* psi200_im, const double ab[4], const bk_gmres_opts* lsopts,
                          bk_precond* pl, double* h30_re, double* h30_im, double* h21_re, double* h21_im, double* h31_re,
                          double* h31_im, double* h22, double g[5], int* converged, int itlinear[4]) {
    const double* const ins[8] = {x, z_re, z_im, zs_re, zs_im, psi110, psi200_re, psi200_im};
    double* const outs[7] = {h30_re, h30_im, h21_re, h21_im, h31_re, h31_im, h22};
    const double* const outsc[7] = {h30_re, h30_im, h21_re, h21_im, h31_re, h31_im, h22};
    if (!ctx || !prob || !params || !ab || !lsopts || !g || any_null(ins) || any_null(outsc)) return -1;
    BK_TRY(minaug_check(ctx, prob, "bautin normal form"));
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, 0, &c));
    BK_TRY(check_alias(ctx, "bk_bautin_normal_form", ins, outs));
    // <zeta, zeta*> = 1 (:721-722): Q = zeta*^H zeta of bk_hopf_contract is its conjugate
    double pq[4];
    BK_TRY(bk_hopf_contract(prob, x, params, nparams, 0, z_re, z_im, zs_re, zs_im, 0, nullptr, pq));
    if (!(std::hypot(pq[2] - 1.0, pq[3]) <= 1e-8))
        return set_error(ctx, "bk_bautin_normal_form: Error of precision in normalization: <zeta, zeta*> = %.17g%+.17gi, expected 1",
                         pq[2], -pq[3]);
    const size_t n = prob->nloc;
    WsGuard ws(ctx);
    double* w[6];       // H20 = 2 Psi200 (re, im), then the right-hand sides of two solves at a time
    for (double*& p : w) BK_TRY(ws.get(n, &p));
    double *h20r = w[0], *h20i = w[1];
    BK_TRY(v_axpbyz(ctx, n, 2.0, psi200_re, 0.0, psi200_re, h20r));
    BK_TRY(v_axpbyz(ctx, n, 2.0, psi200_im, 0.0, psi200_im, h20i));
    const double g21[2] = {2.0 * ab[2], -2.0 * ab[3]};                       // G21 = 2 conj(b)
    JPair jp;
    BK_TRY(jp.make(prob, x, params, nparams));
    // H30, H21
    BK_TRY(v_bautin_rhs3(ctx, n, c, {x, z_re, z_im, h20r, h20i, psi110}, g21, {w[2], w[3], w[4], w[5]}));
    int cv30 = 0, it30 = 0, cv21 = 0, it21[2] = {0, 0}, cv31 = 0, it31 = 0;
    double dl[2];
    BK_TRY(bk_gmres_cshift(ctx, jp.J, w[2], w[3], h30_re, h30_im, 0.0, 3.0 * omega, -1.0, lsopts, pl, &cv30, &it30, nullptr));
    if (minaug_hopf_bordered(ctx)) {                // J - i omega is singular here: the bordered system in ONE preconditioned solve
        GmresResult r21;
        BK_TRY(minaug_hopf_bordered_solve(ctx, jp.J, z_re, z_im, zs_re, zs_im, w[4], w[5], 0.0, -omega, *lsopts, pl, h21_re, h21_im,
                                          dl, &r21));
        cv21 = r21.converged;
        it21[0] = r21.niter;
    } else {
        BK_TRY(bk_bls_bordering_cshift(ctx, jp.J, z_re, z_im, zs_re, zs_im, 0.0, 0.0, w[4], w[5], 0.0, 0.0, 1.0, 1.0, 0.0, -omega, 1.0,
                                       lsopts, pl, h21_re, h21_im, dl, &cv21, it21));
    }
    // H31, H22
    BK_TRY(v_bautin_rhs4(ctx, n, c, {x, z_re, z_im, h20r, h20i, psi110, h30_re, h30_im, h21_re, h21_im}, g21, {w[2], w[3], w[4]}));
    BK_TRY(bk_gmres_cshift(ctx, jp.J, w[2], w[3], h31_re, h31_im, 0.0, 2.0 * omega, -1.0, lsopts, pl, &cv31, &it31, nullptr));
    GmresResult r22;
    BK_TRY(linsolve(ctx, jp.J, w[4], h22, 0.0, 1.0, *lsopts, pl, &r22));
    BK_TRY(v_scale(ctx, n, -1.0, h22));
    ctx->diag.bautin_unconverged += (cv30 ? 0.0 : 1.0) + (cv21 ? 0.0 : 1.0) + (cv31 ? 0.0 : 1.0) + (r22.converged ? 0.0 : 1.0);
    BK_TRY(v_bautin_contract(ctx, n, c, {x, z_re, z_im, zs_re, zs_im, h20r, h20i, psi110, h30_re, h30_im, h21_re, h21_im, h31_re,
                                         h31_im, h22}, g + 2));
    g[0] = g21[0];
    g[1] = g21[1];
    g[4] = g[2] / 12.0;
    if (converged) *converged = cv30 & cv21 & cv31 & r22.converged;
    if (itlinear) { itlinear[0] = it30; itlinear[1] = it21[0] + it21[1]; itlinear[2] = it31; itlinear[3] = r22.niter; }
    return 0;
}

}  // extern "C"
