// What the gap behind a v_mfma_f64_4x4x4f64 hides: one wave alone on its SIMD, the product in VGPR form as an asm statement (the form of
// MPC_MM in mpc_wave.hpp), 0..4 independent instructions of one kind behind every product.  Two streams:
//   independent: eight accumulator chains, product i of a trip extends chain i;
//   dependent:   one chain, every product reads the one before it as srcA and srcC (the recursion of the tile sweeps), six wait states
//                apart as the DGEMM hazard asks: the fillers count as wait states, s_nop makes up the rest.
// A trip is eight products and three scalar instructions of loop control.  The LDS kinds wait (lgkmcnt(0)) after every fourth product,
// twice a trip: with four fillers per gap a trip issues 32 LDS operations and the counter holds 15.
// No ds_read2_b64 row: the pair lands in four consecutive registers, and the sweeps keep the two blocks of a field in operands of
// their own (f[d], f[d + 1] of mpc_wave.hpp), read by different statements; splitting a quad costs the moves this table prices.
// Printed: cycles (s_memtime) per product.
#include <hip/hip_runtime.h>
#include <cstdio>

#define MM "v_mfma_f64_4x4x4_4b_f64 "
#define F_FMA(i) "v_fma_f64 %[f" #i "], %[c], %[c], %[f" #i "]\n\t"
#define F_DPP(i) "v_mov_b32_dpp %[g" #i "], %[src] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" \
                 "v_mov_b32_dpp %[g" #i "], %[src] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t"
#define F_RD(i) "ds_read_b64 %[r" #i "], %[addr] offset:" #i "*512\n\t"
#define F_WR(i) "ds_write_b64 %[addr], %[c] offset:" #i "*512\n\t"
#define F_NOP(i) "s_nop 0\n\t"
#define F_SALU(i) "s_add_u32 %[s], %[s], 1\n\t"
#define F_MM(i) MM "%[y" #i "], %[a], %[b], %[y" #i "]\n\t"
#define GAP0(F) ""
#define GAP1(F) F(0)
#define GAP2(F) F(0) F(1)
#define GAP3(F) F(0) F(1) F(2)
#define GAP4(F) F(0) F(1) F(2) F(3)
// s_nop that completes six wait states behind n fillers of one (P1) or two (P2) instructions
#define P1_0 "s_nop 5\n\t"
#define P1_1 "s_nop 4\n\t"
#define P1_2 "s_nop 3\n\t"
#define P1_3 "s_nop 2\n\t"
#define P1_4 "s_nop 1\n\t"
#define P2_0 "s_nop 5\n\t"
#define P2_1 "s_nop 3\n\t"
#define P2_2 "s_nop 1\n\t"
#define P2_3 ""
#define P2_4 ""
#define IND(i, G) MM "%[x" #i "], %[a], %[b], %[x" #i "]\n\t" G
#define IND_TRIP(G, W) IND(0, G) IND(1, G) IND(2, G) IND(3, G) W IND(4, G) IND(5, G) IND(6, G) IND(7, G) W
#define DEP2(G, P) MM "%[x1], %[x0], %[b], %[x0]\n\t" G P MM "%[x0], %[x1], %[b], %[x1]\n\t" G P
#define DEP_TRIP(G, P, W) DEP2(G, P) DEP2(G, P) W DEP2(G, P) DEP2(G, P) W
#define OPS : [x0] "+v"(x[0]), [x1] "+v"(x[1]), [x2] "+v"(x[2]), [x3] "+v"(x[3]), [x4] "+v"(x[4]), [x5] "+v"(x[5]), [x6] "+v"(x[6]), [x7] "+v"(x[7]), \
              [f0] "+v"(f[0]), [f1] "+v"(f[1]), [f2] "+v"(f[2]), [f3] "+v"(f[3]), [g0] "+v"(g[0]), [g1] "+v"(g[1]), [g2] "+v"(g[2]), [g3] "+v"(g[3]), \
              [r0] "+v"(r[0]), [r1] "+v"(r[1]), [r2] "+v"(r[2]), [r3] "+v"(r[3]), [y0] "+v"(y[0]), [y1] "+v"(y[1]), [y2] "+v"(y[2]), [y3] "+v"(y[3]), [s] "+s"(s) \
            : [a] "v"(a), [b] "v"(b), [c] "v"(c), [src] "v"(src), [addr] "v"(addr) : "scc", "memory"
#define CASE(K, n, F, P, W) \
    if constexpr (KIND == K && NF == n) { if (DEP) asm volatile(DEP_TRIP(GAP##n(F), P, W) OPS); else asm volatile(IND_TRIP(GAP##n(F), W) OPS); }
#define CASES(K, F, PW, W) CASE(K, 0, F, PW##_0, W) CASE(K, 1, F, PW##_1, W) CASE(K, 2, F, PW##_2, W) CASE(K, 3, F, PW##_3, W) CASE(K, 4, F, PW##_4, W)
#define LGKM "s_waitcnt lgkmcnt(0)\n\t"

static const char *const kKind[] = {"v_fma_f64", "v_mov_b32 dpp pair", "ds_read_b64", "ds_write_b64", "s_nop 0", "s_add_u32", "independent product"};

template <int KIND, int NF, bool DEP>
__global__ void __launch_bounds__(64) k(double *out, unsigned long long *cyc, int iters)
{
    __shared__ double lds[64 + 4 * 64];
    const int l = threadIdx.x;
    lds[l] = l; lds[64 + l] = l; lds[128 + l] = l; lds[192 + l] = l; lds[256 + l] = l;
    __syncthreads();
    double x[8], f[4], r[4], y[4];
    const double a = 1.0 + 1e-9 * l, b = 1e-3 * (l & 3), c = 1.0 - 1e-9 * l;
    for (int i = 0; i < 8; i++) x[i] = 1e-3 * l + i;
    for (int i = 0; i < 4; i++) { f[i] = 1e-3 * l + i; r[i] = 0.0; y[i] = 1e-3 * l - i; }
    int g[4] = {l, l + 1, l + 2, l + 3}, src = l, s = iters;
    const unsigned addr = (unsigned)(size_t)lds + 8u * l;       // the low 32 bits of a __shared__ address are its LDS offset
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; it++) {
        CASES(0, F_FMA, P1, "") CASES(1, F_DPP, P2, "") CASES(2, F_RD, P1, LGKM) CASES(3, F_WR, P1, LGKM)
        CASES(4, F_NOP, P1, "") CASES(5, F_SALU, P1, "") CASES(6, F_MM, P1, "")
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    __syncthreads();
    double sum = lds[l + 64] + s;
    for (int i = 0; i < 8; i++) sum += x[i];
    for (int i = 0; i < 4; i++) sum += f[i] + r[i] + g[i] + y[i];
    out[l] = sum;
    if (l == 0) cyc[0] = t1 - t0;
}

static double *g_out;
static unsigned long long *g_cyc;

template <int KIND, int NF, bool DEP>
double run()
{
    const int iters = 2000;
    unsigned long long h = 0;
    for (int rep = 0; rep < 2; rep++) hipLaunchKernelGGL((k<KIND, NF, DEP>), dim3(1), dim3(64), 0, 0, g_out, g_cyc, iters);
    if (hipMemcpy(&h, g_cyc, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
    return (double)h / (iters * 8.0);
}

template <int KIND, bool DEP>
void row()
{
    printf("%-11s %-20s %7.1f %7.1f %7.1f %7.1f %7.1f\n", DEP ? "dependent" : "independent", kKind[KIND],
           run<KIND, 0, DEP>(), run<KIND, 1, DEP>(), run<KIND, 2, DEP>(), run<KIND, 3, DEP>(), run<KIND, 4, DEP>());
}

template <bool DEP>
void table()
{
    row<0, DEP>(); row<1, DEP>(); row<2, DEP>(); row<3, DEP>(); row<4, DEP>(); row<5, DEP>(); row<6, DEP>();
}

int main()
{
    if (hipMalloc(&g_out, 64 * sizeof(double)) != hipSuccess || hipMalloc(&g_cyc, 64) != hipSuccess) return 1;
    printf("cycles per product, fillers per gap:         0       1       2       3       4\n");
    table<false>(); table<true>();
    (void)hipFree(g_out); (void)hipFree(g_cyc);
    return 0;
}
