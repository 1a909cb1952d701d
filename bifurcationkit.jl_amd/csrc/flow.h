// What flow.hip (the spectral ETDRK2 flow of cGL and its tangent) and shooting.hip (the standard-shooting functional on it) share:
// the flow handle and the one marching routine every entry goes through.
// Internal header.
#pragma once
#include <cmath>

#include "cgl_pw.h"
#include "common.h"
#include "ops.h"

struct bk_flow {
    bk_ctx* ctx = nullptr;
    bk_problem* prob = nullptr;
    int B = 0;                     // trajectories that advance in lock-step
    int nx = 0, ny = 0;
    size_t n = 0;                  // grid points per field; a trajectory holds N = 2 n doubles
    bk::DctPlan* plan1 = nullptr;  // DST-I of 2 B fields: the state alone, or the tangent alone
    bk::DctPlan* plan2 = nullptr;  // ... of 4 B fields: state and tangent in one march (created with the first such march)
    bk::DctPlan* last = nullptr;   // the plan of the last march (bk_flow_transform_paths)
    double* tab = nullptr;         // [3 n]: E | h phi1 | h phi2 of the step tab_h
    double tab_h = 0.0;
    bool tab_set = false;
    double* work = nullptr;        // [6][2 B N]
    long long base_marches = 0;    // marches that advanced the state (kFlowBase, kFlowBoth), since creation
    long long launches = 0;        // kernels launched by flow_march since creation
    size_t len() const { return 2 * n * (size_t)B; }
};

namespace bk {

// kFlowBase: the state alone (optionally recording u_n and a_n of every step in physical space); kFlowBoth: state and tangent in one
// march; kFlowTangent: the tangent alone on a recorded base trajectory.  The tangent's arithmetic is the same code in the last two,
// on the same base values: the same bits.
enum FlowMode { kFlowBase = 0, kFlowBoth = 1, kFlowTangent = 2 };

// The problem kind and parameter count, as the Hopf / potrap entries check them (flow.hip)
int flow_params(bk_problem* prob, const double* params, int nparams, CglPar* par);
int flow_create(bk_problem* prob, int B, const char* who, bk_flow** out);
void flow_destroy(bk_flow* f);
// nsteps steps of h = tau / nsteps from x (and dx).  out (kFlowBase, kFlowBoth) = the states, dout (kFlowBoth, kFlowTangent) = the
// tangents, B N doubles each.  store_u, store_a (kFlowBase, both or neither): nsteps B N doubles each, step s at s B N -- u_s and the
// stage value a_s; base_u, base_a (kFlowTangent): what such a march recorded, step s at s * base_stride (0: B N; a march of one
// trajectory on the record of a wider one passes the wider stride).
int flow_march(bk_flow* f, FlowMode mode, const CglPar& par, const double* x, const double* dx, double tau, int nsteps, double* out,
               double* dout, double* store_u, double* store_a, const double* base_u, const double* base_a, size_t base_stride = 0);

}  // namespace bk
