// sk_probe.hip — element-wise probes of the step engine's numeric primitives
// (TEST INFRASTRUCTURE ONLY, never linked into libskillshot).
//
// The product headers are included unchanged and every primitive is wrapped in
// a plain element-wise loop: element i of each input array goes through the
// product function and what it returns is stored at element i of each output
// array.  No arithmetic of its own.  One source, two builds (oracle/Makefile):
//
//   hipcc, the product's flag list      -> _build/libsk_probe.so: one kernel per
//       group, one thread per element, bounds-checked; skp_<group>(args, n,
//       stream) takes DEVICE pointers and returns hipGetLastError()'s status
//   g++ -O2 -std=c++17 -ffp-contract=off -> _build/libsk_probe_host.so: the same
//       wrappers of the host-compilable headers (sk_trig.hpp, sk_tan_cr.hpp,
//       sk_range.hpp) as a loop over HOST pointers; skp_<group>_host(args, n)
//
// A group's arguments are a struct of pointers, inputs first; the field order is
// restated in oracle/probe.py (GROUPS).  Arrays are flat, n elements each; an
// array of k-tuples is k planes of n (element i of plane j at [j * n + i]).
#include <stdint.h>

#if defined(__HIPCC__)
#include "../skillshot_learning_amd/csrc/sk_device.hpp"
#else
#include "../skillshot_learning_amd/csrc/sk_tan_cr.hpp"
#include "../skillshot_learning_amd/csrc/sk_trig.hpp"
#endif
#include "../skillshot_learning_amd/csrc/sk_range.hpp"

#if defined(__HIPCC__)
#define SKP_HD __host__ __device__ __forceinline__
#define SKP_D __device__ __forceinline__
#else
#define SKP_HD static inline
#endif

// ---------------------------------------------------------------- trig (host + device)
struct skp_trig_args {
  const double* x;       // the angle
  const float* d;        // sincos_add's step
  const float* speed;    // fast_move_delta's / fast_step_delta's speed
  const float* act;      // fast_move_delta's (clamped) action
  const float* rs_d;     // round_safe(rs_d, rs_eps)
  const float* rs_eps;
  const double* look;    // look_fits_add
  double *bf_s, *bf_c;          // sincos_bf(x)
  float *fast_s, *fast_c;       // sincos_fast(x)
  float *add_s, *add_c;         // sincos_add(sincos_fast(x), d)
  float *move_x, *move_y;       // fast_move_delta(sincos_fast(x), ok, speed, act)
  float *step_x, *step_y;       // fast_step_delta(sincos_add(sincos_fast(x), d), ok, speed)
  uint8_t *bf_ok, *fast_ok, *rs, *move_safe, *step_safe, *look_fits;
};

SKP_HD void skp_trig_one(const skp_trig_args& a, int64_t i) {
  bool ok_bf, ok;
  const sktrig::SinCos b = sktrig::sincos_bf(a.x[i], &ok_bf);
  const sktrig::SinCosF f = sktrig::sincos_fast(a.x[i], &ok);
  const sktrig::SinCosF g = sktrig::sincos_add(f, a.d[i]);
  const sktrig::FastDelta m = sktrig::fast_move_delta(f, ok, a.speed[i], a.act[i]);
  const sktrig::FastDelta q = sktrig::fast_step_delta(g, ok, a.speed[i]);
  a.bf_s[i] = b.s; a.bf_c[i] = b.c; a.bf_ok[i] = ok_bf;
  a.fast_s[i] = f.s; a.fast_c[i] = f.c; a.fast_ok[i] = ok;
  a.add_s[i] = g.s; a.add_c[i] = g.c;
  a.move_x[i] = m.x; a.move_y[i] = m.y; a.move_safe[i] = m.safe;
  a.step_x[i] = q.x; a.step_y[i] = q.y; a.step_safe[i] = q.safe;
  a.rs[i] = sktrig::round_safe(a.rs_d[i], a.rs_eps[i]);
  a.look_fits[i] = sktrig::look_fits_add(a.look[i]);
}

// ---------------------------------------------------------------- tan
struct skp_tan_args {
  const double* x;
  double* tan_cr;                           // sktan::tan_cr(x)            (host + device)
  double *grad_cr, *grad_fast, *tan_lib;    // sk::grad_cr(x), sk::grad_fast(x), sk::tan_lib(x)  (device only)
};

// ---------------------------------------------------------------- the library past the fast range (device only)
struct skp_lib_args {
  const double* x;
  double *s, *c;  // sk::sincos_lib(x)
};

// ---------------------------------------------------------------- range (host + device)
// v: 8 planes of int; every predicate reads the leading values of the tuple.
// out: 11 planes of u8 in the order below.
struct skp_range_args {
  const int* v;
  uint8_t* out;
};
enum { SKP_RANGE_IN = 8, SKP_RANGE_OUT = 11 };

SKP_HD void skp_range_one(const skp_range_args& a, int64_t n, int64_t i) {
  int v[SKP_RANGE_IN];
  for (int k = 0; k < SKP_RANGE_IN; ++k) v[k] = a.v[k * n + i];
  const skrange::PairHit ph = skrange::pair_hit(v[0] != 0, v[1] != 0, v[2] != 0);
  a.out[0 * n + i] = skrange::cfg_ok(v[0], v[1], v[2], v[3], v[4], v[5]);
  a.out[1 * n + i] = skrange::fits_axis(v[0], v[1]);
  a.out[2 * n + i] = skrange::fits_board(v[0], v[1], v[2], v[3]);
  a.out[3 * n + i] = skrange::box_hit(v[0], v[1], v[2], v[3], v[4], v[5]);
  a.out[4 * n + i] = ph.h1;
  a.out[5 * n + i] = ph.h2;
  a.out[6 * n + i] = skrange::pack_fits_player(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
  a.out[7 * n + i] = skrange::pack_fits_game(v[0], v[1], v[2]);
  a.out[8 * n + i] = skrange::admit_cfg(v[0], v[1], v[2], v[3], v[4]);
  a.out[9 * n + i] = skrange::admit_player(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
  a.out[10 * n + i] = skrange::admit_game(v[0], v[1], v[2], v[3]);
}

// ---------------------------------------------------------------- features (device only)
struct skp_feat_args {
  const double* r;   // py_mod2(r), py_mod2_fast(r)
  const int* p;      // 4 planes: dist_point_point(p0, p1, p2, p3), dist_line_point(g, p0, p1, p2, p3)
  const double* g;
  const double* a;   // clamp_action(a)
  const float* af;   // clamp_action_f(af)
  double *mod2, *mod2_fast, *dpp, *dlp, *clamp;
  float* clamp_f;
};

// ---------------------------------------------------------------- rng (device only)
struct skp_rng_args {
  const uint32_t* ctr;   // 4 planes
  const uint32_t* key;   // 2 planes
  const uint32_t* u;     // u32_to_action(u), u32_to_pos(u, lo, hi)
  const int *lo, *hi;
  uint32_t* out;         // 4 planes: philox4x32_10(ctr, key)
  float* action;
  int* pos;
};

#if defined(__HIPCC__)

SKP_D void skp_tan_one(const skp_tan_args& a, int64_t i) {
  a.tan_cr[i] = sktan::tan_cr(a.x[i]);
  a.grad_cr[i] = sk::grad_cr(a.x[i]);
  a.grad_fast[i] = sk::grad_fast(a.x[i]);
  a.tan_lib[i] = sk::tan_lib(a.x[i]);
}

SKP_D void skp_lib_one(const skp_lib_args& a, int64_t i) {
  const sktrig::SinCos t = sk::sincos_lib(a.x[i]);
  a.s[i] = t.s;
  a.c[i] = t.c;
}

SKP_D void skp_feat_one(const skp_feat_args& a, int64_t n, int64_t i) {
  const int p0 = a.p[0 * n + i], p1 = a.p[1 * n + i], p2 = a.p[2 * n + i], p3 = a.p[3 * n + i];
  a.mod2[i] = sk::py_mod2(a.r[i]);
  a.mod2_fast[i] = sk::py_mod2_fast(a.r[i]);
  a.dpp[i] = sk::dist_point_point(p0, p1, p2, p3);
  a.dlp[i] = sk::dist_line_point(a.g[i], p0, p1, p2, p3);
  a.clamp[i] = sk::clamp_action(a.a[i]);
  a.clamp_f[i] = sk::clamp_action_f(a.af[i]);
}

SKP_D void skp_rng_one(const skp_rng_args& a, int64_t n, int64_t i) {
  const sk::U4 c = {a.ctr[0 * n + i], a.ctr[1 * n + i], a.ctr[2 * n + i], a.ctr[3 * n + i]};
  const sk::U4 o = sk::philox4x32_10(c, a.key[0 * n + i], a.key[1 * n + i]);
  a.out[0 * n + i] = o.x; a.out[1 * n + i] = o.y; a.out[2 * n + i] = o.z; a.out[3 * n + i] = o.w;
  a.action[i] = sk::u32_to_action(a.u[i]);
  a.pos[i] = sk::u32_to_pos(a.u[i], a.lo[i], a.hi[i]);
}

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ int64_t element() { return (int64_t)blockIdx.x * kBlock + threadIdx.x; }

__global__ void __launch_bounds__(kBlock) k_probe_trig(skp_trig_args a, int64_t n) {
  const int64_t i = element();
  if (i < n) skp_trig_one(a, i);
}
__global__ void __launch_bounds__(kBlock) k_probe_tan(skp_tan_args a, int64_t n) {
  const int64_t i = element();
  if (i < n) skp_tan_one(a, i);
}
__global__ void __launch_bounds__(kBlock) k_probe_lib(skp_lib_args a, int64_t n) {
  const int64_t i = element();
  if (i < n) skp_lib_one(a, i);
}
__global__ void __launch_bounds__(kBlock) k_probe_range(skp_range_args a, int64_t n) {
  const int64_t i = element();
  if (i < n) skp_range_one(a, n, i);
}
__global__ void __launch_bounds__(kBlock) k_probe_feat(skp_feat_args a, int64_t n) {
  const int64_t i = element();
  if (i < n) skp_feat_one(a, n, i);
}
__global__ void __launch_bounds__(kBlock) k_probe_rng(skp_rng_args a, int64_t n) {
  const int64_t i = element();
  if (i < n) skp_rng_one(a, n, i);
}

// n elements at most 2^31 - 1 blocks' worth; nothing to launch for n <= 0
inline bool grid_of(int64_t n, unsigned* blocks) {
  if (n <= 0 || n > (int64_t)kBlock * 0x7fffffff) return false;
  *blocks = (unsigned)((n + kBlock - 1) / kBlock);
  return true;
}

}  // namespace

#define SKP_LAUNCHER(group, kernel)                                                        \
  extern "C" int skp_##group(const skp_##group##_args* a, int64_t n, hipStream_t stream) { \
    unsigned blocks;                                                                       \
    if (n == 0) return (int)hipSuccess;                                                    \
    if (!a || !grid_of(n, &blocks)) return (int)hipErrorInvalidValue;                      \
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream, *a, n);              \
    return (int)hipGetLastError();                                                         \
  }

SKP_LAUNCHER(trig, k_probe_trig)
SKP_LAUNCHER(tan, k_probe_tan)
SKP_LAUNCHER(lib, k_probe_lib)
SKP_LAUNCHER(range, k_probe_range)
SKP_LAUNCHER(feat, k_probe_feat)
SKP_LAUNCHER(rng, k_probe_rng)

#else  // the host twin

extern "C" int skp_trig_host(const skp_trig_args* a, int64_t n) {
  for (int64_t i = 0; i < n; ++i) skp_trig_one(*a, i);
  return 0;
}
extern "C" int skp_tan_host(const skp_tan_args* a, int64_t n) {  // tan_cr alone: the rest is device-only
  for (int64_t i = 0; i < n; ++i) a->tan_cr[i] = sktan::tan_cr(a->x[i]);
  return 0;
}
extern "C" int skp_range_host(const skp_range_args* a, int64_t n) {
  for (int64_t i = 0; i < n; ++i) skp_range_one(*a, n, i);
  return 0;
}

#endif
