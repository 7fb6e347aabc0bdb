// Host code the three libraries share underneath their C ABIs (mpc_amd.hip, mpc_nmpc.hip, mpc_enmpc.hip): the error state, device buffers,
// the padded structure-of-arrays staging and the table of the closed loop's logs.  Host only, header only, everything static: each library
// (each translation unit) gets its own copy, nothing is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

// ---------------------------------------------------------------------------------------------------
// error handling: the message *_last_error returns; -10 = a HIP call failed (-12, an RCCL call: mpc_comm.hpp)
// ---------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(x)                                                                                       \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) return fail(-10, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    int ensure(size_t n)
    {
        if (n <= bytes) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        HIP_TRY(hipMalloc(&p, n));
        bytes = n;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// batch padded to whole waves: the stride of one row of a device array
static size_t pad64(size_t b) { return (b + 63) / 64 * 64; }

// host [B][d] -> SoA staging [d][Bs], the padding lanes zero
static void to_soa(const double *src, int B, int d, size_t Bs, double *dst)
{
    for (int i = 0; i < d; i++) {
        double *row = dst + (size_t)i * Bs;
        for (int b = 0; b < B; b++) row[b] = src[(size_t)b * d + i];
        for (size_t b = B; b < Bs; b++) row[b] = 0.0;
    }
}
// host [nsteps][B][d] -> staging [step][d][Bs]: per-instance values of every step of a resident loop (its white noise), step by step through to_soa
static void steps_to_soa(const double *src, int nsteps, int B, int d, size_t Bs, double *dst)
{
    for (int k = 0; k < nsteps; k++) to_soa(src + (size_t)k * B * d, B, d, Bs, dst + (size_t)k * d * Bs);
}
static void from_soa(const double *src, int B, int d, size_t Bs, double *dst)
{
    for (int i = 0; i < d; i++) {
        const double *row = src + (size_t)i * Bs;
        for (int b = 0; b < B; b++) dst[(size_t)b * d + i] = row[b];
    }
}

// ---------------------------------------------------------------------------------------------------
// The logs of a resident closed loop: float64 logs [step][dim][Bs] one after the other in `dbl`, int32 logs [which][step][Bs] in `ints`.
// Which logs exist, how many of their steps are valid and what a missing one is called are the caller's.
// ---------------------------------------------------------------------------------------------------
struct LogTab {
    struct Entry { size_t off; int dim; };      // offset in doubles / ints; dim 0 = an int32 log
    std::map<std::string, Entry> at;
    size_t n_dbl = 0, n_int = 0, Bs = 0;         // doubles / ints of the two device arrays
    int max_steps = 0;
    DevBuf dbl, ints;

    // the layout alone (no HIP call): float64 log j behind its predecessors, max_steps * dim * Bs doubles each (every dim > 0: a log of dimension
    // zero is the caller's to leave out); int32 log i at i * max_steps * Bs
    void layout(const std::vector<std::pair<const char *, int>> &dlogs, const std::vector<const char *> &ilogs, int max_steps_, size_t Bs_)
    {
        at.clear();
        max_steps = max_steps_; Bs = Bs_; n_dbl = 0;
        for (const auto &l : dlogs) { at[l.first] = {n_dbl, l.second}; n_dbl += (size_t)max_steps * l.second * Bs; }
        for (size_t i = 0; i < ilogs.size(); i++) at[ilogs[i]] = {i * max_steps * Bs, 0};
        n_int = ilogs.size() * max_steps * Bs;
    }
    int alloc() { return (dbl.ensure(n_dbl ? n_dbl * 8 : 8) || (n_int && ints.ensure(n_int * 4))) ? -10 : 0; }
    void release() { dbl.release(); ints.release(); }

    const Entry *find(const char *name) const { auto it = at.find(name); return it == at.end() ? nullptr : &it->second; }
    // device address of step k of a log (double * or int32_t * by its kind), nullptr for a log that does not exist
    void *dev(const char *name, int k = 0) const
    {
        const Entry *e = find(name);
        if (!e) return nullptr;
        if (e->dim > 0) return (double *)dbl.p + e->off + (size_t)k * e->dim * Bs;
        return (int32_t *)ints.p + e->off + (size_t)k * Bs;
    }
    // steps [k0, k0 + n) of a float64 log as they lie on the device: n * dim * Bs doubles from *src
    int slice(const Entry &e, int k0, int n, const double **src, size_t *count) const
    {
        if (k0 < 0 || n < 1 || k0 + n > max_steps) return fail(-1, "steps out of range");
        *src = (const double *)dbl.p + e.off + (size_t)k0 * e.dim * Bs;
        *count = (size_t)n * e.dim * Bs;
        return 0;
    }
    // the first ns steps of a log to the host: [ns][B][dim] float64, [ns][B] int32 (blocking copy: the caller has synchronised its stream)
    int read(const Entry &e, int ns, int B, void *out) const
    {
        if (e.dim > 0) {
            std::vector<double> st((size_t)ns * e.dim * Bs);
            HIP_TRY(hipMemcpy(st.data(), (const double *)dbl.p + e.off, st.size() * 8, hipMemcpyDeviceToHost));
            unpad(st.data(), ns, e.dim, B, Bs, (double *)out);
        } else {
            std::vector<int32_t> st((size_t)ns * Bs);
            HIP_TRY(hipMemcpy(st.data(), (const int32_t *)ints.p + e.off, st.size() * 4, hipMemcpyDeviceToHost));
            for (int k = 0; k < ns; k++) for (int b = 0; b < B; b++) ((int32_t *)out)[(size_t)k * B + b] = st[(size_t)k * Bs + b];
        }
        return 0;
    }
    // host copy of `blocks` steps [dim][Bs] -> [blocks][B][dim] (a gathered [world][n][dim][Bs] block: blocks = world * n)
    static void unpad(const double *st, size_t blocks, int dim, int B, size_t Bs, double *out)
    {
        for (size_t k = 0; k < blocks; k++) from_soa(st + k * dim * Bs, B, dim, Bs, out + k * B * dim);
    }
};

#ifdef MPC_STAMPS
// diagnostic builds only: read (out, n words) and / or clear a __device__ array of cycle stamps
template <size_t N>
static int debug_stamps(unsigned long long (&sym)[N], unsigned long long *out, int n, int reset)
{
    if (out) { if (hipMemcpyFromSymbol(out, HIP_SYMBOL(sym), sizeof(unsigned long long) * n) != hipSuccess) return -1; }
    if (reset) { static unsigned long long z[N]; if (hipMemcpyToSymbol(HIP_SYMBOL(sym), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#endif
