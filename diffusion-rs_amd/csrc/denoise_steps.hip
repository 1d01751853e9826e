// denoise_steps.hip — the denoise loop's per-step update of the state: Euler, the Heun predictor and corrector, DPM-Solver++ 2M.
// One kernel frame (step_kernel) owns what every update shares: the grid-stride pass, 16-byte accesses when every operand allows them and scalar ones
// otherwise, the guided velocity under true CFG and the inpainting blend.  An update is an operation struct: its own pointers and scalars, its own arithmetic.
// Every product that feeds a sum is an explicit fmaf, so an expression rounds the same in every instantiation and the tests can count its roundings.
// A new solver's step: one operation struct and one launcher that hands it to launch_step.
#include <cmath>
#include <type_traits>

#include "common.h"

namespace fmi {

namespace {
template <int W>
__device__ __forceinline__ void ld(const float* __restrict__ p, int64_t i, float (&r)[W]) {
  if constexpr (W == 4) {
    const float4 t = reinterpret_cast<const float4*>(p)[i];
    r[0] = t.x, r[1] = t.y, r[2] = t.z, r[3] = t.w;
  } else {
    r[0] = p[i];
  }
}
template <int W>
__device__ __forceinline__ void st(float* p, int64_t i, const float (&r)[W]) {
  if constexpr (W == 4)
    reinterpret_cast<float4*>(p)[i] = make_float4(r[0], r[1], r[2], r[3]);
  else
    p[i] = r[0];
}
// what a step walks along: the prediction, or under CFG neg + scale * (pos - neg) — the difference first, diffusers' expression: pos == neg or scale == 0 gives
// neg bit for bit
template <bool CFG>
__device__ __forceinline__ float guided(float pos, float neg, float scale) {
  if constexpr (CFG) return fmaf(scale, pos - neg, neg);
  return pos;
}
// the blend of a state e at time s: m = 1 gives e and m = 0 gives k = a * x0 + s * noise bit for bit (finite inputs)
__device__ __forceinline__ float blend_at(float e, float x0, float noise, float m, float a, float s) {
  const float k = fmaf(a, x0, s * noise);
  const float keep = 1.0f - m;
  return fmaf(m, e, keep * k);
}
// What every update reads besides its own operands.  neg: null without guidance; x0 / noise / mask: all three or none.
struct StepArgs {
  const float *pos, *neg;
  float scale;
  const float *x0, *noise, *mask;
  float a, s;  // s: the target time of the blend, a = 1 - s
};
// The blend operands of one item, and the blend of a state with them: the identity without BLEND (the arrays are then never written or read).
template <int W, bool BLEND>
struct Blend {
  float x0[W], z[W], m[W], a, s;
  __device__ __forceinline__ float operator()(float e, int j) const {
    if constexpr (BLEND) return blend_at(e, x0[j], z[j], m[j], a, s);
    return e;
  }
};

// The operations.  op.apply<W>(i, g, blend): item i's update along the velocity g — the state a step leaves is blended, whatever else it writes is not.
// aligned(): every operand of its own allows 16-byte accesses.  A buffer is read and written at the same index only.
// img = img + g * dt  (pipelines/sampling.rs:43; the latent is kept in f32)
struct EulerOp {
  float* img;
  float dt;
  bool aligned() const { return all_aligned16({img}); }
  template <int W, class B>
  __device__ __forceinline__ void apply(int64_t i, const float (&g)[W], const B& blend) const {
    float x[W], o[W];
    ld<W>(img, i, x);
#pragma unroll
    for (int j = 0; j < W; ++j) o[j] = blend(fmaf(g[j], dt, x[j]), j);
    st<W>(img, i, o);
  }
};
// xt = img + g * dt, g1 = g: Euler's state into a second buffer.  The state itself is only read.
struct HeunPredictOp {
  const float* img;
  float *xt, *g1;
  float dt;
  bool aligned() const { return all_aligned16({img, xt, g1}); }
  template <int W, class B>
  __device__ __forceinline__ void apply(int64_t i, const float (&g)[W], const B& blend) const {
    float x[W], o[W];
    ld<W>(img, i, x);
#pragma unroll
    for (int j = 0; j < W; ++j) o[j] = blend(fmaf(g[j], dt, x[j]), j);
    st<W>(xt, i, o), st<W>(g1, i, g);
  }
};
// img = img + ((g1 + g) * 0.5) * dt; g1 == g gives the Euler step along g1 bit for bit
struct HeunCorrectOp {
  float* img;
  const float* g1;
  float dt;
  bool aligned() const { return all_aligned16({img, g1}); }
  template <int W, class B>
  __device__ __forceinline__ void apply(int64_t i, const float (&g)[W], const B& blend) const {
    float x[W], f[W], o[W];
    ld<W>(img, i, x), ld<W>(g1, i, f);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float h = (f[j] + g[j]) * 0.5f;
      o[j] = blend(fmaf(h, dt, x[j]), j);
    }
    st<W>(img, i, o);
  }
};
// D = img - t * g;  D' = D + w * (D - hist) (w == 0: D' = D and hist is not read);  img = a * img + c * D';  hist = D
struct Dpmpp2mOp {
  float *img, *hist;
  float t, a, c, w;
  bool aligned() const { return all_aligned16({img, hist}); }
  template <int W, class B>
  __device__ __forceinline__ void apply(int64_t i, const float (&g)[W], const B& blend) const {
    float x[W], h[W], d[W], o[W];
    ld<W>(img, i, x);
    if (w != 0.f) ld<W>(hist, i, h);  // (uniform over the grid)
#pragma unroll
    for (int j = 0; j < W; ++j) {
      d[j] = fmaf(-t, g[j], x[j]);
      const float dp = w != 0.f ? fmaf(w, d[j] - h[j], d[j]) : d[j];
      o[j] = blend(fmaf(a, x[j], c * dp), j);
    }
    st<W>(img, i, o), st<W>(hist, i, d);
  }
};

// W = 4 (16-byte accesses; n counts float4s) or 1 (any alignment, any n).  Without CFG neg, and without BLEND x0 / noise / mask, are never touched (null then).
template <int W, bool CFG, bool BLEND, class Op>
__global__ __launch_bounds__(256) void step_kernel(Op op, StepArgs c, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float p[W], q[W], g[W];
    Blend<W, BLEND> blend;
    ld<W>(c.pos, i, p);
    if constexpr (CFG) ld<W>(c.neg, i, q);
    if constexpr (BLEND) ld<W>(c.x0, i, blend.x0), ld<W>(c.noise, i, blend.z), ld<W>(c.mask, i, blend.m), blend.a = c.a, blend.s = c.s;
#pragma unroll
    for (int j = 0; j < W; ++j) g[j] = guided<CFG>(p[j], q[j], c.scale);
    op.template apply<W>(i, g, blend);
  }
}

template <class F>
void with_flag(bool b, F f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
// One of an operation's eight instantiations: 16-byte accesses when n % 4 == 0 and every pointer that instantiation touches is 16-byte aligned, else scalar;
// guided when neg is not null; blended with x0 / noise / mask (all three or none: `who` names the refusing entry).
template <class Op>
int launch_step(const char* who, const Op& op, const float* pos, const float* neg, float scale, int64_t n, hipStream_t stream, const float* x0, const float* noise,
                const float* mask, float s) {
  const bool blend = x0 && noise && mask;
  if (!blend && (x0 || noise || mask)) return fail(FMI_ERR_INVALID, std::string(who) + ": x0, noise and mask go together (all three or none)");
  if (n <= 0) return FMI_OK;
  const bool v4 = n % 4 == 0 && op.aligned() && all_aligned16({pos, neg, x0, noise, mask});
  const int64_t items = v4 ? n / 4 : n;
  const StepArgs c{pos, neg, scale, x0, noise, mask, 1.0f - s, s};
  with_flag(v4, [&](auto V4) {
    with_flag(neg != nullptr, [&](auto CFG) {
      with_flag(blend, [&](auto BLEND) {
        hipLaunchKernelGGL((step_kernel<decltype(V4)::value ? 4 : 1, decltype(CFG)::value, decltype(BLEND)::value, Op>), map_grid(items), dim3(256), 0, stream, op, c, items);
      });
    });
  });
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}
}  // namespace

int launch_euler_step(float* img, const float* pos, const float* neg, float scale, float dt, int64_t n, hipStream_t stream, const float* x0, const float* noise,
                      const float* mask, float s) {
  return launch_step("cfg_euler_step", EulerOp{img, dt}, pos, neg, scale, n, stream, x0, noise, mask, s);
}
int launch_heun_predict(const float* img, const float* pos, const float* neg, float scale, float dt, int64_t n, float* xt, float* g1, hipStream_t stream, const float* x0,
                        const float* noise, const float* mask, float s) {
  return launch_step("heun_predict", HeunPredictOp{img, xt, g1, dt}, pos, neg, scale, n, stream, x0, noise, mask, s);
}
int launch_heun_correct(float* img, const float* g1, const float* pos, const float* neg, float scale, float dt, int64_t n, hipStream_t stream, const float* x0,
                        const float* noise, const float* mask, float s) {
  return launch_step("heun_correct", HeunCorrectOp{img, g1, dt}, pos, neg, scale, n, stream, x0, noise, mask, s);
}
// a, c, w: dpmpp_2m_coefficients; t: the step's time
int launch_dpmpp_2m(float* img, const float* pos, const float* neg, float scale, float t, float a, float c, float w, int64_t n, float* hist, hipStream_t stream,
                    const float* x0, const float* noise, const float* mask, float s) {
  return launch_step("dpmpp_2m_step", Dpmpp2mOp{img, hist, t, a, c, w}, pos, neg, scale, n, stream, x0, noise, mask, s);
}

// A solver's schedule: ts[0..n_steps] strictly decreasing inside [0, 1] (NaN fails every comparison).
int check_solver_schedule(const double* ts, int n_steps, const char* who) {
  if (!ts || n_steps < 0) return fail(FMI_ERR_INVALID, std::string(who) + ": null schedule or negative n_steps");
  if (!(ts[0] <= 1.0) || !(ts[n_steps] >= 0.0)) return fail(FMI_ERR_INVALID, std::string(who) + ": a solver's schedule lies in [0, 1] (1 >= ts[0], ts[n_steps] >= 0)");
  for (int i = 0; i < n_steps; ++i)
    if (!(ts[i + 1] < ts[i])) return fail(FMI_ERR_INVALID, std::string(who) + ": a solver's schedule is strictly decreasing");
  return FMI_OK;
}
// Step i's scalars of DPM-Solver++ 2M under flow matching (sigma = t, alpha = 1 - t, lambda = ln((1 - t) / t)), in f64 and rounded once:
//   a = t_{i+1} / t_i, c = 1 - a, w = (l_{i+1} - l_i) / (2 (l_i - l_{i-1})) — and w = 0 without history, after t_{i-1} == 1 and into t_{i+1} == 0.
void dpmpp_2m_coefficients(const double* ts, int i, float* a, float* c, float* w) {
  const double t0 = ts[i], t1 = ts[i + 1], ad = t1 / t0;
  double wd = 0.0;
  if (i > 0 && ts[i - 1] != 1.0 && t1 != 0.0) {
    const auto lam = [](double t) { return std::log((1.0 - t) / t); };
    wd = (lam(t1) - lam(t0)) / (2.0 * (lam(t0) - lam(ts[i - 1])));
  }
  *a = (float)ad, *c = (float)(1.0 - ad), *w = (float)wd;
}

}  // namespace fmi

using namespace fmi;

// ------------------------------------------------------------------ C-ABI: the updates on their own.  The launcher refuses a partial x0 / noise / mask.
extern "C" int fmi_cfg_euler_step(float* img, const float* pos, const float* neg, float scale, float dt, int64_t n, const float* x0, const float* noise,
                                  const float* mask, float s, void* stream) {
  if (!img || !pos || !neg || n < 0) return fail(FMI_ERR_INVALID, "cfg_euler_step: bad arguments");
  if (!(scale >= 0.f) || std::isinf(scale)) return fail(FMI_ERR_INVALID, "cfg_euler_step: scale must be finite and >= 0");
  return launch_euler_step(img, pos, neg, scale, dt, n, (hipStream_t)stream, x0, noise, mask, s);
}
// The solvers' updates.  neg NULL: no guidance, scale is not looked at.
static int check_solver_step(const char* who, const void* neg, float scale, int64_t n) {
  if (n < 0) return fail(FMI_ERR_INVALID, std::string(who) + ": n must not be negative");
  if (neg && (!(scale >= 0.f) || std::isinf(scale))) return fail(FMI_ERR_INVALID, std::string(who) + ": scale must be finite and >= 0");
  return FMI_OK;
}
extern "C" int fmi_heun_predict(const float* img, const float* pos, const float* neg, float scale, float dt, int64_t n, float* x_pred, float* g1, const float* x0,
                                const float* noise, const float* mask, float s, void* stream) {
  if (!img || !pos || !x_pred || !g1) return fail(FMI_ERR_INVALID, "heun_predict: null img / pos / x_pred / g1");
  if (x_pred == img || g1 == img || x_pred == g1) return fail(FMI_ERR_INVALID, "heun_predict: img, x_pred and g1 are three buffers");
  FMI_TRY(check_solver_step("heun_predict", neg, scale, n));
  return launch_heun_predict(img, pos, neg, scale, dt, n, x_pred, g1, (hipStream_t)stream, x0, noise, mask, s);
}
extern "C" int fmi_heun_correct(float* img, const float* g1, const float* pos, const float* neg, float scale, float dt, int64_t n, const float* x0, const float* noise,
                                const float* mask, float s, void* stream) {
  if (!img || !g1 || !pos) return fail(FMI_ERR_INVALID, "heun_correct: null img / g1 / pos");
  if (g1 == img) return fail(FMI_ERR_INVALID, "heun_correct: img and g1 are two buffers");
  FMI_TRY(check_solver_step("heun_correct", neg, scale, n));
  return launch_heun_correct(img, g1, pos, neg, scale, dt, n, (hipStream_t)stream, x0, noise, mask, s);
}
extern "C" int fmi_dpmpp_2m_step(float* img, const float* pos, const float* neg, float scale, float t, float a, float c, float w, int64_t n, float* history,
                                 const float* x0, const float* noise, const float* mask, float s, void* stream) {
  if (!img || !pos || !history) return fail(FMI_ERR_INVALID, "dpmpp_2m_step: null img / pos / history");
  if (history == img) return fail(FMI_ERR_INVALID, "dpmpp_2m_step: img and history are two buffers");
  FMI_TRY(check_solver_step("dpmpp_2m_step", neg, scale, n));
  return launch_dpmpp_2m(img, pos, neg, scale, t, a, c, w, n, history, (hipStream_t)stream, x0, noise, mask, s);
}
extern "C" int fmi_dpmpp_2m_coefficients(const double* timesteps_host, int n_steps, int i, float* a, float* c, float* w) {
  if (!a || !c || !w) return fail(FMI_ERR_INVALID, "dpmpp_2m_coefficients: null output");
  FMI_TRY(check_solver_schedule(timesteps_host, n_steps, "dpmpp_2m_coefficients"));
  if (i < 0 || i >= n_steps) return fail(FMI_ERR_INVALID, "dpmpp_2m_coefficients: step i outside [0, n_steps)");
  dpmpp_2m_coefficients(timesteps_host, i, a, c, w);
  return FMI_OK;
}
