// stp3_sampler.hip -- the planner's candidate set: the trajectory sampler of the reference's data loaders for gfx950.
//
// Replaces, behind stp3_traj_sample, stp3/utils/sampler.py:8-146 as NuscenesData.get_trajectory_sampling (:389-437) and the
// CARLA loader call it: per sample M trajectories -- straight lines, arcs about the (clamped) measured curvature and clothoids
// through the Fresnel integrals -- drawn around the measured speed, of which the loaders keep the n_future + 1 poses at the
// frame times t_k = k dt ([:, ::10]).  Only those poses are evaluated here (pose 0 is the clothoid's origin, the last pose
// carries the sort key).  The random stream is an INPUT: `draws` holds the uniforms in the order the reference consumes its
// numpy stream, so the same draws give the reference's trajectories.
//
// One workgroup per sample, one launch per batch.  A thread owns a trajectory ("generation index" g: the row of the
// reference's array before its sort, [left | lines | right], :142): it evaluates the last pose and writes a 64-bit key into
// LDS -- the lateral position rounded to float32 (the value that is stored) above g, so that equal positions order by
// generation index: a total order, no atomics, and the reference's accident of numpy among its ~M/5 exactly tied straight
// lines becomes a rule.  A bitonic network sorts the keys in LDS (66 barriers for 1 800 rows; counting ranks by all
// pairs took half of the kernel's time), then the thread of output row r evaluates all poses of the trajectory ranked r.
//
// Arithmetic: float64 in the reference's operation order (the library is built with -ffp-contract=off), one rounding to
// float32 on the store: the clothoid heading pi/2 x^2 reaches ~255 rad and positions ~75 m, float32 trigonometry there is
// 1e-5 off.  Fresnel S(x), C(x): |x| < 2: the Maclaurin series in t = pi x^2 / 2 (22 terms by Horner's rule, coefficients
// in LDS; the largest term is e^t ~ 535, so cancellation costs < 1e-13); |x| >= 2: C = 1/2 + f sin t - g cos t, S = 1/2 - f cos t - g sin t with the auxiliary functions
// from their Laplace integrals (DLMF 7.7.10-11), which after s -> u / a, a = x sqrt(pi / 2), are Gaussian-weighted integrals of
// the smooth 1 / (1 + (u/a)^4) and (u/a)^2 / (1 + (u/a)^4): the trapezoidal rule with step 0.3 on 21 nodes converges
// geometrically (the integrand's poles lie 0.886 x >= 1.77 off the real axis: error ~ e^{-2 pi 1.77 / 0.3}).  Measured
// against scipy.special.fresnel on [-16, 16]: 2e-15 (tests/test_sampler_cpu.py holds it to 1e-9 on the stored grid).
// stp3_amd/ops_plan.py restates the same method and constants in torch (sample_trajectories_reference).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "stp3_hip.h"

namespace {

// Keeps a wave-uniform value in a vector register (an empty statement: no instruction is issued).  The kernel's float64
// constants compete for the 102 scalar registers; the per-sample values and pointers below would be spilled from them.
#if defined(__HIP_DEVICE_COMPILE__)
#define STP3_IN_VGPR(x) asm volatile("" : "+v"(x))
#else
#define STP3_IN_VGPR(x) (void)(x)
#endif

constexpr int kThreads = 1024;               // 4 waves per SIMD of one CU (96 VGPRs, no spills, no scratch)
constexpr int kMaxM = 8192;                  // keys: 8 bytes each in 64 KB of LDS
constexpr double kPi = 3.141592653589793;
constexpr double kFresnelSplit = 2.0;
constexpr double kFresnelStep = 0.3;
constexpr int kFresnelNodes = 21;
constexpr int kFresnelTerms = 22;

struct SamplerDims {
    int B, M, nl, ns, nr, T;                 // T = n_future + 1 poses
    int P;                                   // M rounded up to a power of two
    double dt;
    int sort;
};

// The tables of one workgroup (LDS): w[k] = exp(-(k step)^2), and the Maclaurin coefficients
// cc[n] = (-1)^n / ((2n)! (4n + 1)), cs[n] = (-1)^n / ((2n + 1)! (4n + 3)) with the factorial as a running float64 product
// (stp3_amd/ops_plan.py builds the same numbers by the same operations).
struct FresnelTables {
    double w[kFresnelNodes + 1], cc[kFresnelTerms], cs[kFresnelTerms];
};

__device__ __forceinline__ void fill_tables(FresnelTables& tab, int tid) {
    if (tid <= kFresnelNodes) {
        const double u = (double)tid * kFresnelStep;
        tab.w[tid] = exp(-(u * u));
    }
    if (tid < kFresnelTerms) {
        double f = 1.0;                                   // (2 tid)!
        for (int k = 2; k <= 2 * tid; ++k) f = f * (double)k;
        const double sign = (tid & 1) ? -1.0 : 1.0;
        tab.cc[tid] = sign / (f * (double)(4 * tid + 1));
        tab.cs[tid] = sign / (f * (double)(2 * tid + 1) * (double)(4 * tid + 3));
    }
}

// S(x), C(x); the caller hands over t = pi x^2 / 2 and its sine / cosine (it evaluates them once for everything a pose needs)
__device__ __forceinline__ void fresnel(double x, double t, double sn, double cn, const FresnelTables& tab, double& s, double& c) {
    const double ax = fabs(x);
    if (ax < kFresnelSplit) {                             // C = x sum cc[n] t^2n, S = x t sum cs[n] t^2n (Horner)
        const double t2 = t * t;
        double pc = tab.cc[kFresnelTerms - 1], ps = tab.cs[kFresnelTerms - 1];
#pragma unroll 1
        for (int n = kFresnelTerms - 2; n >= 0; --n) {
            pc = pc * t2 + tab.cc[n];
            ps = ps * t2 + tab.cs[n];
        }
        c = ax * pc;
        s = ax * (t * ps);
    } else {
        const double a = ax * sqrt(kPi / 2.0), inv_a = 1.0 / a;
        double f = 0.5, g = 0.0;
#pragma unroll 1
        for (int k = 1; k <= kFresnelNodes; ++k) {
            const double r = ((double)k * kFresnelStep) * inv_a, s2 = r * r;
            const double d = 1.0 / (1.0 + s2 * s2);
            f = f + tab.w[k] * d;
            g = g + tab.w[k] * s2 * d;
        }
        const double scale = sqrt(2.0) / kPi * kFresnelStep * inv_a;
        f = f * scale;
        g = g * scale;
        c = 0.5 + f * sn - g * cn;
        s = 0.5 - f * cn - g * sn;
    }
    if (x < 0.0) { s = -s; c = -c; }
}

// sin and cos of one angle.  Not inlined: the constants of the argument reduction would otherwise be held in scalar registers
// over the whole kernel (39 of them spilled).
struct SinCos { double s, c; };
__device__ __attribute__((noinline)) SinCos sin_cos(double a) {
    SinCos r;
    sincos(a, &r.s, &r.c);
    return r;
}

// numpy's float remainder for a positive divisor, then the shift: (theta + pi) % (2 pi) - pi  (sampler.py:65, :101)
__device__ __forceinline__ double wrap(double theta) {
    double r = fmod(theta + kPi, 2.0 * kPi);
    if (r < 0.0) r += 2.0 * kPi;
    else if (r == 0.0) r = 0.0;              // (-0.0 -> +0.0, as numpy)
    return r - kPi;
}

// the draws of one trajectory
struct Row {
    double acc, vel, alpha;
    int kind;                                // 0 line, 1 arc, 2 clothoid
    bool mirror;
};

struct Sample {
    double v0, kappa, inv_kr, xi0;
};

__device__ __forceinline__ Sample sample_of(double v0, double kappa) {
    Sample p;
    p.v0 = v0;
    p.kappa = kappa;
    const double kr = kappa <= 0.0 ? fmin(-0.01, kappa) : fmax(0.01, kappa);        // :53
    p.inv_kr = 1.0 / kr;                                                            // radius = |1 / kr|, centre x = -1 / kr
    p.xi0 = fabs(kappa) / kPi;                                                      // :72
    STP3_IN_VGPR(p.v0); STP3_IN_VGPR(p.kappa); STP3_IN_VGPR(p.inv_kr); STP3_IN_VGPR(p.xi0);
    return p;
}

__device__ __forceinline__ Row row_of(const SamplerDims& d, const Sample& p, const double* __restrict__ draws, int g) {
    // generation index -> row of the reference's draw arrays (:129-142)
    const bool left_first = p.kappa > 0.0;
    const int first = left_first ? d.nl : d.nr;           // length of the block in front of the lines
    int line = -1, j = 0;
    Row r;
    r.mirror = false;
    if (g < first) {
        j = left_first ? g : d.nl + g;
        r.mirror = !left_first;
    } else if (g < first + d.ns) {
        line = g - first;
    } else {
        j = left_first ? g - d.ns : g - first - d.ns;
        r.mirror = left_first;
    }
    const int m = line >= 0 ? line : d.ns + j;            // L_straight = L[:straight_num], the curves take the rest (:38-39)
    const int M = d.M, Mc = d.nl + d.nr;
    r.acc = 10.0 * (draws[m] - 0.5) + 2.0;                // :28
    r.vel = draws[2 * M + m] >= 0.2 ? 15.0 * draws[M + m] : p.v0;                   // :32-34
    r.kind = 0;
    r.alpha = 1.0;
    if (line >= 0) return r;
    r.alpha = (80.0 - 6.0) * draws[3 * M + j] + 6.0;      // :43
    r.kind = draws[3 * M + Mc + j] >= 0.2 ? 2 : 1;        // :109
    return r;
}

// The poses k_first .. T - 1 of one trajectory, stored to `out` (when given); returns the stored x of the last pose.
// One loop serves everything that needs a sine / cosine or a Fresnel pair, so that each is in the code once: step -2 the
// clothoid's start rotation (:84-92), step -1 its origin (the pose at L = 0, :82-83), steps 0 .. T - 1 the poses.
__device__ __forceinline__ float eval_row(const SamplerDims& d, const Sample& p, const Row& r, const FresnelTables& w,
                                          int k_first, float* __restrict__ out) {
    const double radius = fabs(p.inv_kr), cx = -p.inv_kr;
    const bool arc_pos = p.inv_kr >= 0.0;
    const double n0x = p.kappa <= 0.0 ? 1.0 : -1.0;                                 // N0 of the loaders
    const double sign = p.kappa > 0.0 ? 1.0 : p.kappa < 0.0 ? -1.0 : p.kappa;       // np.sign: 0 -> 0, NaN -> NaN
    const double q0 = p.kappa / kPi / r.alpha;
    const double theta0 = 0.5 * kPi * (q0 * q0);                                    // :84
    double px0 = 0.0, py0 = 0.0, rot_s = 0.0, rot_c = 1.0;
    float last = 0.f;
#pragma unroll 1
    for (int k = -2; k < d.T; ++k) {
        if (k >= 0 && k < k_first) continue;
        if (k < 0 && r.kind != 2) continue;
        const double t = k > 0 ? d.dt * (double)k : 0.0;
        const double L = r.vel * t + r.acc * (t * t) / 2.0;                         // :37
        const double q = L / radius;
        const double phi = arc_pos ? q : kPi - q;
        const double arg = (p.xi0 + L) / r.alpha, aarg = fabs(arg);
        const double tf = 0.5 * kPi * aarg * aarg;
        const double angle = k == -2 ? theta0 * sign : r.kind == 1 ? phi : tf;
        const SinCos sc = sin_cos(angle);
        const double sn = sc.s, cn = sc.c;
        if (k == -2) { rot_s = sn; rot_c = cn; continue; }
        double x, y, theta;
        if (r.kind == 0) {                                // :47-49
            x = L * 0.0;
            y = L * 1.0;
            theta = 0.0;
        } else if (r.kind == 1) {                         // :53-66
            x = cx + radius * cn;
            y = 0.0 + radius * sn;
            theta = arc_pos ? q : -q;
        } else {                                          // :72-101
            double s, c;
            fresnel(arg, tf, sn, cn, w, s, c);
            const double px = r.alpha * (c * 0.0 + s * n0x);                        // :79, T0 = (0, 1), N0 = (n0x, 0)
            const double py = r.alpha * (c * 1.0 + s * 0.0);
            if (k == -1) { px0 = px; py0 = py; continue; }
            const double xs = px - px0, ys = py - py0;
            x = rot_c * xs + rot_s * ys;
            y = -rot_s * xs + rot_c * ys;
            theta = (0.5 * kPi * (arg * arg) - theta0) * sign;
        }
        theta = wrap(theta);                              // (a line's 0 stays 0)
        if (r.mirror) { x = -x; theta = -theta; }         // :132-134, :138-140
        if (out) {
            out[3 * k] = (float)x;
            out[3 * k + 1] = (float)y;
            out[3 * k + 2] = (float)theta;
        }
        last = (float)x;
    }
    return last;
}

__global__ __launch_bounds__(kThreads) void traj_sample_kernel(SamplerDims d, const double* __restrict__ v0,
                                                               const double* __restrict__ kappa,
                                                               const double* __restrict__ draws, float* __restrict__ trajs,
                                                               int* __restrict__ order) {
    extern __shared__ __attribute__((aligned(16))) uint64_t keys[];
    __shared__ FresnelTables w;
    const int b = blockIdx.x, tid = threadIdx.x;
    fill_tables(w, tid);
    __syncthreads();
    const Sample p = sample_of(v0[b], kappa[b]);
    const double* dr = draws + (size_t)b * (3 * d.M + 2 * (d.nl + d.nr));
    STP3_IN_VGPR(order); STP3_IN_VGPR(trajs); STP3_IN_VGPR(dr);
    // phase 0 (sort only): the keys; phase 1: the rows.  One loop, so that the row evaluation is in the code once.
#pragma unroll 1
    for (int phase = d.sort ? 0 : 1; phase < 2; ++phase) {
        if (phase == 1 && d.sort) {
            // bitonic sorting network over the P slots; the thread of the lower slot of a pair does the exchange
            __syncthreads();
            for (int k = 2; k <= d.P; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < d.P; i += kThreads) {
                        const int l = i ^ j;
                        if (l > i) {
                            const uint64_t lo = keys[i], hi = keys[l];
                            if ((lo > hi) == ((i & k) == 0)) { keys[i] = hi; keys[l] = lo; }
                        }
                    }
                    __syncthreads();
                }
        }
        const int n = phase == 0 ? d.P : d.M;
        for (int i = tid; i < n; i += kThreads) {
            // phase 0: slot i = generation index i (slots from M up pad the power of two and sort behind every row);
            // phase 1: output row i <- the trajectory of that rank
            if (i >= d.M) { keys[i] = ~0ull; continue; }
            const int g = (phase == 1 && d.sort) ? (int)(uint32_t)keys[i] : i;
            const Row r = row_of(d, p, dr, g);
            float* out = phase == 1 ? trajs + ((size_t)b * d.M + i) * d.T * 3 : nullptr;
            const float x = eval_row(d, p, r, w, phase == 1 ? 0 : d.T - 1, out);
            if (phase == 0) {
                // 64-bit key: the stored float32 x of the last pose as an order-preserving unsigned integer (-0 counts as +0)
                // above the generation index -- all different, so their order is the ordering rule and nothing else
                const uint32_t bits = __float_as_uint(x + 0.0f);
                keys[i] = ((uint64_t)((bits & 0x80000000u) ? ~bits : bits | 0x80000000u) << 32) | (uint32_t)g;
            } else if (order) {
                order[(size_t)b * d.M + i] = g;
            }
        }
    }
}

}  // namespace

extern "C" {

int stp3_traj_sample(const stp3_sampler_dims* p, const double* v0, const double* kappa, const double* draws, float* trajs,
                     int32_t* order, void* stream) {
    if (!p || p->B < 1 || p->M < 1 || p->n_future < 1 || p->n_left < 0 || p->n_straight < 0 || p->n_right < 0 ||
        (int64_t)p->n_left + p->n_straight + p->n_right != p->M || !(p->dt > 0.0) || !v0 || !kappa || !draws || !trajs)
        return STP3_EINVAL;
    if (p->M > kMaxM) return STP3_EUNSUP;
    SamplerDims d;
    d.B = p->B; d.M = p->M; d.nl = p->n_left; d.ns = p->n_straight; d.nr = p->n_right; d.T = p->n_future + 1;
    d.dt = p->dt; d.sort = p->sort;
    d.P = 1;
    while (d.P < d.M) d.P <<= 1;
    hipLaunchKernelGGL(traj_sample_kernel, dim3(p->B), dim3(kThreads), d.sort ? (size_t)d.P * sizeof(uint64_t) : 0,
                       (hipStream_t)stream, d, v0, kappa, draws, trajs, order);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? STP3_OK : -(int)e;
}

}  // extern "C"
