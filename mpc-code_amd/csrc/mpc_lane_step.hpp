// The closed-loop step of the instance-per-lane kernels of mpc_amd.hip, one function per phase (MPC_code.py:485-827): launch state, logs,
// measure and estimate, target, slab fill of the def_px / def_py form, accept or hold, plant step (the hard OCP solve between them stays in the
// kernels, see lane_ws) - and the input load /
// result store of the per-call OCP kernels.  loop_kernel, loop_kernel_soft and loop_kernel_pxy are sequences of these calls around what is
// their own; ocp_kernel, ocp_kernel_soft, ocp_kernel_pxy and kf_kernel take the parts they share with the loops from here, which is what
// makes a fused run the call-by-call one bit for bit.  Plain function templates on register arrays, every one inlined.
//
// loop_kernel_tp (and loop_kernel_wv) keep their own copies of the scalar phases on purpose: loop_kernel_tp addresses the loop state as
// (ptr + i * Bs)[bq] with an index made opaque once per step and splits the Kalman step over two waves, loop_kernel_wv works on lanes of
// several instances at once.  An edit to a phase below has to be repeated there by hand.
#pragma once
#include "../../include/mpc_amd.h"
#include "mpc_device.hpp"
#ifdef MPC_NL_PLANT_HEADER
// A non-linear plant for the fused closed loop (Ex_LMPC_nlplant.py, Ex_LMPCxp_nlplant.py: linear controller, User_fxp_Cont as the
// simulated process): struct NlPlant { NXP, NU, MX; __device__ static void f(x, u, t, xdot); } generated from the traced Ex-file
// function (mpc-code_amd/nlcodegen.py:emit_plant_header); a library built with it carries exactly one dimension set.
#include MPC_NL_PLANT_HEADER
#endif

struct OcpArgs {
    const double *xhat, *xs, *us, *dhat, *u_prev;   // in
    double *u_out, *xnext_out, *res;                // out ([nu][Bs], [nx][Bs], [3][Bs])
    int32_t *status, *iters;
    double *ws;                                     // workspace rows
    int B; size_t Bs;
};

// The closed loop, MPC_code.py:485-827: `nsteps` consecutive steps per launch, state read from / written
// back to HBM once per launch.
struct LoopArgs {
    double *x, *xhat, *dhat, *Pk, *u, *xs, *us;      // state [dim][Bs]
    const double *ysp, *usp, *pxp, *pyp;             // schedules [step][dim], already offset to k0
    double *U, *XHAT, *XS, *US, *YS, *XP, *DHAT;     // logs [step][dim][Bs] offset to k0, or nullptr
    int32_t *st_dyn, *st_ss, *it_dyn, *it_ss;        // logs [step][Bs] offset to k0, or nullptr
    int32_t *ws_valid;                               // [Bs] 1 if the workspace holds a solved OCP of the previous step
    int32_t *kf_valid;                               // [Bs] 1 if Kg / Pn hold the filter gain of this step and the prior after it
    double *Kg, *Pn;                                 // [ne*ny][Bs], [ne*ne][Bs] (horizon-parallel kernel: computed one step ahead)
    double *tw; int32_t *tw_valid;                   // warm start of the target solve: [2*(nu-nh_ss) + 3*(nx+nu+ny+ng_ss)][Bs], [Bs]
    double *ws;
    int B, nsteps; size_t Bs;
    int N;                                           // horizon (host side: sizes the dynamic LDS of the wave-autonomous kernel)
    double t0, h;                                    // time of the launch's first step, sampling interval (a user plant integrates in time)
    int wv_ni;                                       // wave-autonomous kernel: instances per wave (0 = by batch size; option "wave_instances")
    const double *px_h, *py_h;                       // def_px / def_py over the horizon, [step][N][nx] / [step][N][ny] offset to k0 (loop_kernel_pxy), or nullptr
    double *lin;                                     // loop_kernel_pxy: slab of per-block stage data
    double *SL, *soft_ws, *sl_keep;                  // loop_kernel_soft: log of the slacks [step][2 ny][Bs] offset to k0 (or nullptr), the arrowhead solver's workspace, the last accepted slacks [2 ny][Bs]
    const double *vn, *wn;                           // white noise per step and instance (mpc_loop_set_noise), [step][ny][Bs] on the measurement and [step][nxp][Bs] on the
                                                     // plant state after its step, offset to k0; nullptr: none (MPC_code.py:537-541, 822-827).  The fields above keep their places
    const double *ysp_b, *usp_b;                     // set points per step and instance (mpc_loop_set_setpoints), [step][ny][Bs] / [step][nu][Bs], offset to k0; nullptr: that quantity
                                                     // is the shared schedule's (ysp / usp above).  Last: the fields above keep their places
};

namespace mpc {

// x_p(t + h) (MPC_code.py:813-816).  Linear plant: Ap x + Bp u + pxp (Utilities.py:45-49).  User plant: MX classical RK4 steps of
// dx/dt = f(x, u, t) over h with the inputs held and time carried along, then + pxp (Utilities.py:58-82, casadi.simpleRK; LinPar).
template <int NXP, int NU, class PT>
__device__ __forceinline__ void plant_next(const PT &P, const double (&x)[NXP], const double (&u)[NU], const double *pxp_k, double t, double h, double (&xn)[NXP])
{
#ifdef MPC_NL_PLANT_HEADER
    static_assert(NlPlant::NXP == NXP && NlPlant::NU == NU, "the plant header belongs to another dimension set");
    (void)P;
    const double dt = h / NlPlant::MX;
    double xx[NXP];
    MPC_UNROLL for (int i = 0; i < NXP; i++) xx[i] = x[i];
    for (int s = 0; s < NlPlant::MX; s++) {
        const double ts = t + s * dt;
        double k1[NXP], k2[NXP], k3[NXP], k4[NXP], xa[NXP];
        NlPlant::f(xx, u, ts, k1);
        MPC_UNROLL for (int i = 0; i < NXP; i++) xa[i] = xx[i] + 0.5 * dt * k1[i];
        NlPlant::f(xa, u, ts + 0.5 * dt, k2);
        MPC_UNROLL for (int i = 0; i < NXP; i++) xa[i] = xx[i] + 0.5 * dt * k2[i];
        NlPlant::f(xa, u, ts + 0.5 * dt, k3);
        MPC_UNROLL for (int i = 0; i < NXP; i++) xa[i] = xx[i] + dt * k3[i];
        NlPlant::f(xa, u, ts + dt, k4);
        MPC_UNROLL for (int i = 0; i < NXP; i++) xx[i] += dt / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
    }
    MPC_UNROLL for (int i = 0; i < NXP; i++) xn[i] = xx[i] + pxp_k[i];
#else
    (void)t; (void)h;
    MPC_UNROLL for (int i = 0; i < NXP; i++) {
        double v = pxp_k[i];
        MPC_UNROLL for (int j = 0; j < NXP; j++) v += P.Ap[i][j] * x[j];
        MPC_UNROLL for (int j = 0; j < NU; j++) v += P.Bp[i][j] * u[j];
        xn[i] = v;
    }
#endif
}

// ---- launch state: x, xhat, dhat, u and the target, registers <-> HBM once per launch ------------------------------------------------
template <int ND, int NXP, int NX, int NU>
__device__ __forceinline__ void lane_state_load(const LoopArgs &a, int b, double (&x)[NXP], double (&xh)[NX], double *dh, double (&u)[NU], double (&xs)[NX], double (&us)[NU])
{
    const size_t Bs = a.Bs;
    MPC_UNROLL for (int i = 0; i < NXP; i++) x[i] = a.x[i * Bs + b];
    MPC_UNROLL for (int i = 0; i < NX; i++) { xh[i] = a.xhat[i * Bs + b]; xs[i] = a.xs[i * Bs + b]; }
    MPC_UNROLL for (int i = 0; i < ND; i++) dh[i] = a.dhat[i * Bs + b];
    MPC_UNROLL for (int i = 0; i < NU; i++) { u[i] = a.u[i * Bs + b]; us[i] = a.us[i * Bs + b]; }
}

template <int ND, int NXP, int NX, int NU>
__device__ __forceinline__ void lane_state_store(const LoopArgs &a, int b, const double (&x)[NXP], const double (&xh)[NX], const double *dh, const double (&u)[NU], const double (&xs)[NX], const double (&us)[NU])
{
    const size_t Bs = a.Bs;
    MPC_UNROLL for (int i = 0; i < NXP; i++) a.x[i * Bs + b] = x[i];
    MPC_UNROLL for (int i = 0; i < NX; i++) { a.xhat[i * Bs + b] = xh[i]; a.xs[i * Bs + b] = xs[i]; }
    MPC_UNROLL for (int i = 0; i < ND; i++) a.dhat[i * Bs + b] = dh[i];
    MPC_UNROLL for (int i = 0; i < NU; i++) { a.u[i * Bs + b] = u[i]; a.us[i * Bs + b] = us[i]; }
}

// one row of a float log [step][D][Bs] (XP, XHAT, DHAT, XS, US, U), when it is kept
template <int D>
__device__ __forceinline__ void lane_log(double *L, int k, size_t Bs, int b, const double *v)
{
    if (L) { MPC_UNROLL for (int i = 0; i < D; i++) L[((size_t)k * D + i) * Bs + b] = v[i]; }
}

// ---- measure and estimate (MPC_code.py:524-534, 577-668) -----------------------------------------------------------------------------
// The correction of xi = [xhat; dhat] by an innovation: Kalman filter with its covariance [ne*ne][Bs] read and written back, or the fixed
// gain.  (kf_kernel and the loops.)
template <int NE, int NY, class PT>
__device__ __forceinline__ void lane_correct(const PT &P, double *Pk_g, size_t Bs, int b, double (&xi)[NE], const double (&innov)[NY])
{
    if (P.estimator == MPC_EST_KALMAN) {
        double Pk[NE][NE];
        MPC_UNROLL for (int i = 0; i < NE; i++) { MPC_UNROLL for (int j = 0; j < NE; j++) Pk[i][j] = Pk_g[(i * NE + j) * Bs + b]; }
        kalman_lane<NE, NY>(P, xi, Pk, innov);
        MPC_UNROLL for (int i = 0; i < NE; i++) { MPC_UNROLL for (int j = 0; j < NE; j++) Pk_g[(i * NE + j) * Bs + b] = Pk[i][j]; }
    } else if (P.estimator == MPC_EST_FIXED_GAIN) {
        MPC_UNROLL for (int i = 0; i < NE; i++) { double s = 0.0; MPC_UNROLL for (int l = 0; l < NY; l++) s += P.Kfix[i][l] * innov[l]; xi[i] += s; }
    }
}

// One step of the estimator on the plant's output y = Cp x + pyp_k (+ v_k, the white noise a.vn): innovation, correction, saturation of the disturbance estimate.
// py0 (or nullptr): p_y_k of the def_py schedule, in the model's output and in the plant's (p_ymp = p_y_k, MPC_code.py:505-507,534).
template <int NY, int ND, int NXP, int NX, class PT>
__device__ __forceinline__ void lane_estimate(const PT &P, const LoopArgs &a, int k, int b, const double (&x)[NXP], double (&xh)[NX], double *dh, const double *py0 = nullptr)
{
    constexpr int NE = NX + ND;
    if (P.estimator == MPC_EST_NONE) return;
    double xi[NE], innov[NY];
    MPC_UNROLL for (int i = 0; i < NX; i++) xi[i] = xh[i];
    MPC_UNROLL for (int i = 0; i < ND; i++) xi[NX + i] = dh[i];
    MPC_UNROLL for (int i = 0; i < NY; i++) {
        double yh = py0 ? P.fyc[i] + py0[i] : P.fyc[i], yy = a.pyp[k * NY + i];
        if (a.vn) yy += a.vn[((size_t)k * NY + i) * a.Bs + b];
        MPC_UNROLL for (int j = 0; j < NE; j++) yh += P.Ca[i][j] * xi[j];
        MPC_UNROLL for (int j = 0; j < NXP; j++) yy += P.Cp[i][j] * x[j];
        innov[i] = py0 ? (yy + py0[i]) - yh : yy - yh;
    }
    lane_correct<NE, NY>(P, a.Pk, a.Bs, b, xi, innov);
    MPC_UNROLL for (int i = 0; i < NX; i++) xh[i] = xi[i];
    MPC_UNROLL for (int i = 0; i < ND; i++) { double d = xi[NX + i]; if (P.has_dsat) d = dmin(dmax(d, P.dmin[i]), P.dmax[i]); dh[i] = d; }
}

// ---- target (MPC_code.py:693-718): keep the previous one when infeasible; logs XS, US ------------------------------------------------
// warm: the warm-start slot a.tw / a.tw_valid of the target solve (cold, like the per-call entry point, otherwise).  px0 / py0 (or nullptr):
// p_x_k, p_y_k in the equalities; they reach target_lane with or without the warm start.  The set points are the shared schedule's row k, or - a.ysp_b / a.usp_b -
// this instance's own: the only place of these kernels that reads either.
template <int NY, int ND, int NGS, int NHS, int NX, int NU, class PT>
__device__ __forceinline__ int lane_target(const PT &P, const LoopArgs &a, int k, int b, const double *dh, double (&xs)[NX], double (&us)[NU], int &it_ss,
                                           bool warm, const double *px0 = nullptr, const double *py0 = nullptr)
{
    double usp[NU], ysp[NY], xs_n[NX], us_n[NU], ys_n[NY];
    MPC_UNROLL for (int i = 0; i < NU; i++) usp[i] = a.usp[k * NU + i];
    MPC_UNROLL for (int i = 0; i < NY; i++) ysp[i] = a.ysp[k * NY + i];
    if (a.usp_b) { MPC_UNROLL for (int i = 0; i < NU; i++) usp[i] = (a.usp_b + ((size_t)k * NU + i) * a.Bs)[b]; }      // this instance's own set points (mpc_loop_set_setpoints)
    if (a.ysp_b) { MPC_UNROLL for (int i = 0; i < NY; i++) ysp[i] = (a.ysp_b + ((size_t)k * NY + i) * a.Bs)[b]; }
    const int st_ss = target_lane<NX, NU, NY, ND, NGS, NHS>(P, usp, ysp, dh, us, xs_n, us_n, ys_n, it_ss, warm ? a.tw + b : nullptr, warm ? a.Bs : 0,
                                                            warm ? a.tw_valid + b : nullptr, px0, py0);
    if (st_ss != kInfeasible) {
        MPC_UNROLL for (int i = 0; i < NX; i++) xs[i] = xs_n[i];
        MPC_UNROLL for (int i = 0; i < NU; i++) us[i] = us_n[i];
    }
    lane_log<NX>(a.XS, k, a.Bs, b, xs);
    lane_log<NU>(a.US, k, a.Bs, b, us);
    return st_ss;
}

// log YS: ys = Fy_model(xs, us, dhat[, p_y_k]), MPC_code.py:730
template <int NY, int ND, int NX, class PT>
__device__ __forceinline__ void lane_log_ys(const PT &P, const LoopArgs &a, int k, int b, const double (&xs)[NX], const double *dh, const double *py0 = nullptr)
{
    if (!a.YS) return;
    MPC_UNROLL for (int i = 0; i < NY; i++) {
        double v = py0 ? P.fyc[i] + py0[i] : P.fyc[i];
        MPC_UNROLL for (int j = 0; j < NX; j++) v += P.Cm[i][j] * xs[j];
        MPC_UNROLL for (int j = 0; j < ND; j++) v += P.Cd[i][j] * dh[j];
        a.YS[((size_t)k * NY + i) * a.Bs + b] = v;
    }
}

// ---- hard OCP (MPC_code.py:733-805) --------------------------------------------------------------------------------------------------
// this lane's rows of the lane solver's workspace [workgroup][block][slot][64 lanes]
template <int NS, int NU, int NC>
__device__ __forceinline__ Ws lane_ws(double *ws, int N)
{
    constexpr int SL = BlkLayout<NS, NU, NC>::SLOTS;
    return Ws{(gv2d *)((v2d *)ws + ((size_t)blockIdx.x * (N + 2) + 1) * SL * 64), N, SL, (int)threadIdx.x};
}

// The solve itself stays in the kernels: rpdip_lane and, for a terminal equality, up to two more passes - cold - with the terminal reference aimed off
// (mpc_device.hpp:term_aim), a dozen lines in ocp_kernel, ocp_kernel_pxy, loop_kernel and loop_kernel_pxy.  Behind one shared function rpdip_lane has a single
// caller per instantiation, the inliner then pulls it into every kernel, and at the largest dimension sets (stage state 7 and more), where it is called out of
// line, the lane loop was a tenth slower on an MI355X.

// The OCP with model parameters over the horizon (def_px / def_py): the stage-0 output test with py_0 (Control_Calc.py:128-151) into
// q.ok0, and this lane's column of the slab [block][A | B | c_k | lo_k | hi_k][64 lanes] for rpdip_lane<.., LTV>.  px / py (either may be
// null) point at this instance's px_0[0] / py_0[0]; entry (k, i) lies (k * dim + i) * stride further: stride Bs for per-instance
// [N][dim][Bs], 1 for a schedule [N][dim] all instances share.
template <int NX, int NY, int ND, bool DU, int NG, int NS, int NU>
__device__ __forceinline__ void lane_pxy_slab(const DevProblem &P, const StageConst<NS, NU> &C, OcpInst<NS, NU> &q, const double (&xhat)[NX], const double *dh,
                                              const double *px, const double *py, size_t stride, double *lin)
{
    constexpr int NB = NX + (DU ? NU : 0), NLTV = NS * (NS + NU + 1), NLIN = NLTV + 2 * NS;
    const int N = P.N;
    double e0[NY];      // output offsets without py
    MPC_UNROLL for (int i = 0; i < NY; i++) { double e = P.fyc[i]; MPC_UNROLL for (int j = 0; j < ND; j++) e += P.Cd[i][j] * dh[j]; e0[i] = e; }
    if (P.y_bounded && py) {      // the stage-0 row is a test of the given x_0, with py_0
        q.ok0 = true;
        MPC_UNROLL for (int i = 0; i < NY; i++) {
            double y0 = e0[i] + py[(size_t)i * stride];
            MPC_UNROLL for (int j = 0; j < NX; j++) y0 += P.Cm[i][j] * xhat[j];
            const double rl = kBoundRelax * dmax(1.0, fabs(P.ymin[i])), rh = kBoundRelax * dmax(1.0, fabs(P.ymax[i]));
            if (!(y0 >= P.ymin[i] - rl) || !(y0 <= P.ymax[i] + rh)) q.ok0 = false;
        }
    }
    for (int k = 0; k < N; k++) {
        double *lb = lin + (size_t)k * NLIN * 64;
        double pxk[NX];
        MPC_UNROLL for (int i = 0; i < NX; i++) pxk[i] = px ? px[((size_t)k * NX + i) * stride] : 0.0;
        MPC_UNROLL for (int i = 0; i < NS; i++) {
            MPC_UNROLL for (int j = 0; j < NS; j++) lb[(i * NS + j) * 64] = C.A[i][j];
            MPC_UNROLL for (int j = 0; j < NU; j++) lb[(NS * NS + i * NU + j) * 64] = C.B[i][j];
            double c = q.c[i];
            if (i < NX) c += pxk[i < NX ? i : 0];
            if (i >= NB) { const int r = P.yg_row[i >= NB ? i - NB : 0]; MPC_UNROLL for (int j = 0; j < NX; j++) c += P.Cm[r][j] * pxk[j]; }      // w+ = C_i x+
            lb[(NS * NS + NS * NU + i) * 64] = c;
        }
        // bounds of z_{k+1}: the constant boxes, cut by the output rows of stage k + 1 (none at the terminal state)
        double lo[NS], hi[NS];
        const bool end = k == N - 1;
        MPC_UNROLL for (int i = 0; i < NS; i++) { lo[i] = end ? P.zlo_e[i] : P.zlo_m[i]; hi[i] = end ? P.zhi_e[i] : P.zhi_m[i]; }
        if (P.y_bounded && !end) {
            MPC_UNROLL for (int i = 0; i < NY; i++) {
                const double e = e0[i] + (py ? py[((size_t)(k + 1) * NY + i) * stride] : 0.0);
                const double sc = P.ymap_scale[i];
                const double aa = (P.ymin[i] - e) / sc, bb = (P.ymax[i] - e) / sc;
                const double l = sc > 0 ? aa : bb, h = sc > 0 ? bb : aa;
                const int idx = P.ymap_idx[i];
                MPC_UNROLL for (int j = 0; j < NS; j++)
                    if (j == idx) { lo[j] = dmax(lo[j], l); hi[j] = dmin(hi[j], h); }
            }
        }
        MPC_UNROLL for (int i = 0; i < NS; i++) { lb[(NLTV + i) * 64] = lo[i]; lb[(NLTV + NS + i) * 64] = hi[i]; }
    }
}

// ---- accept or hold (MPC_code.py:798-805); logs U and the four status / iteration logs ----------------------------------------------
// the first input of a solved OCP: u_0, or - input v = u - u_prev - the u_prev part of z_1
template <int NX, bool DU, int NS, int NU, class PT>
__device__ __forceinline__ double lane_first_input(const PT &P, const double (&u0)[NU], const double (&z1)[NS], int i)
{
    return (DU && P.in_is_du) ? z1[DU ? NX + i : 0] : u0[i];
}

// u and the prediction of xhat from the OCP's first block; an infeasible OCP holds u and propagates the model (with p_x_k: px0, or nullptr)
template <int ND, bool DU, int NX, int NS, int NU, class PT>
__device__ __forceinline__ void lane_accept_or_hold(const PT &P, const LoopArgs &a, int k, int b, int st_dyn, int st_ss, int it_dyn, int it_ss,
                                                    const double (&u0)[NU], const double (&z1)[NS], double (&u)[NU], double (&xh)[NX], const double *dh, const double *px0 = nullptr)
{
    const size_t Bs = a.Bs;
    if (st_dyn != kInfeasible) {
        MPC_UNROLL for (int i = 0; i < NU; i++) u[i] = lane_first_input<NX, DU>(P, u0, z1, i);          // :798
        MPC_UNROLL for (int i = 0; i < NX; i++) xh[i] = z1[i];         // :799
    } else {                                                           // :804-805
        double xn[NX];
        MPC_UNROLL for (int i = 0; i < NX; i++) {
            double v = px0 ? P.fxc[i] + px0[i] : P.fxc[i];
            MPC_UNROLL for (int j = 0; j < NX; j++) v += P.Am[i][j] * xh[j];
            MPC_UNROLL for (int j = 0; j < NU; j++) v += P.Bm[i][j] * u[j];
            MPC_UNROLL for (int j = 0; j < ND; j++) v += P.Bd[i][j] * dh[j];
            xn[i] = v;
        }
        MPC_UNROLL for (int i = 0; i < NX; i++) xh[i] = xn[i];
    }
    lane_log<NU>(a.U, k, Bs, b, u);
    if (a.st_dyn) { a.st_dyn[(size_t)k * Bs + b] = st_dyn; a.st_ss[(size_t)k * Bs + b] = st_ss; a.it_dyn[(size_t)k * Bs + b] = it_dyn; a.it_ss[(size_t)k * Bs + b] = it_ss; }
}

// ---- plant (MPC_code.py:813-816, 822-827): x <- x_p(t_k + h) (+ w_k, the white noise a.wn); pxp_k is the caller's (the def_px loop adds p_x_k to the schedule's) ----
template <int NXP, int NU, class PT>
__device__ __forceinline__ void lane_plant_step(const PT &P, const LoopArgs &a, int k, int b, double (&x)[NXP], const double (&u)[NU], const double *pxp_k)
{
    double xn[NXP];
    plant_next<NXP, NU>(P, x, u, pxp_k, a.t0 + k * a.h, a.h, xn);
    if (a.wn) { MPC_UNROLL for (int i = 0; i < NXP; i++) xn[i] += a.wn[((size_t)k * NXP + i) * a.Bs + b]; }
    MPC_UNROLL for (int i = 0; i < NXP; i++) x[i] = xn[i];
}

// ---- per-call OCP kernels: input load, result store ----------------------------------------------------------------------------------
template <int ND, int NX, int NU>
__device__ __forceinline__ void ocp_load(const OcpArgs &a, int b, double (&xhat)[NX], double (&xs)[NX], double (&us)[NU], double (&up)[NU], double *dh)
{
    MPC_UNROLL for (int i = 0; i < NX; i++) { xhat[i] = a.xhat[i * a.Bs + b]; xs[i] = a.xs[i * a.Bs + b]; }
    MPC_UNROLL for (int i = 0; i < NU; i++) { us[i] = a.us[i * a.Bs + b]; up[i] = a.u_prev[i * a.Bs + b]; }
    MPC_UNROLL for (int i = 0; i < ND; i++) dh[i] = a.dhat[i * a.Bs + b];
}

template <int NX, bool DU, int NS, int NU, class PT>
__device__ __forceinline__ void ocp_store(const PT &P, const OcpArgs &a, int b, int st, int it, const double (&res)[3], const double (&u0)[NU], const double (&z1)[NS])
{
    a.status[b] = st; a.iters[b] = it;
    MPC_UNROLL for (int i = 0; i < 3; i++) a.res[i * a.Bs + b] = res[i];
    if (st != kInfeasible) {
        MPC_UNROLL for (int i = 0; i < NU; i++) a.u_out[i * a.Bs + b] = lane_first_input<NX, DU>(P, u0, z1, i);
        MPC_UNROLL for (int i = 0; i < NX; i++) a.xnext_out[i * a.Bs + b] = z1[i];
    }
}

}  // namespace mpc
