// Python bindings for the midgpt_amd HIP kernel layer (gfx950).
// Included at the end of ext.hip (single TU — kernel definitions visible).
//
// Every entry point: `Call c("name", first_tensor)` sets the device guard,
// every kernel pointer comes from c.bf16 / c.f32 / c.i64 / c.i32 (which take
// no tensor without a shape), and every kernel goes through launch().
#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <climits>
#include <type_traits>
#include <vector>

static hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// Launch on the current stream; an empty grid launches nothing. Dynamic LDS
// above the 64 KiB default cap (gfx950 has 160 KiB/CU) needs the attribute
// raised first.
template <typename... P, typename... A>
static void launch(void (*kernel)(P...), dim3 grid, int block, size_t smem, A... args) {
  if (grid.x == 0 || grid.y == 0 || grid.z == 0) return;
  if (smem > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    TORCH_CHECK(e == hipSuccess, "cannot raise dynamic LDS to ", smem, " bytes: ",
                hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, grid, dim3(block), smem, cur_stream(), static_cast<P>(args)...);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "HIP launch failed: ", hipGetErrorString(e));
}

// f(integral constant) for a run-time flag, or for a value that is A or else B.
template <typename F>
static void dispatch_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}
template <int A, int B, typename F>
static void dispatch_int(int v, F&& f) {
  if (v == A) f(std::integral_constant<int, A>{});
  else f(std::integral_constant<int, B>{});
}

// What a kernel addresses of a tensor: exact sizes (ANY: a dimension that is
// read from the tensor itself), or with flat(n) the element count alone.
constexpr int64_t ANY = -1;
struct Shape {
  at::IntArrayRef sizes;
  int64_t numel = -1;
  Shape(std::initializer_list<int64_t> s) : sizes(s) {}
  Shape(at::IntArrayRef s) : sizes(s) {}
  bool fits(const torch::Tensor& t) const {
    if (numel >= 0) return t.numel() == numel;
    const at::IntArrayRef ts = t.sizes();
    if (ts.size() != sizes.size()) return false;
    for (size_t i = 0; i < sizes.size(); ++i)
      if (sizes[i] != ANY && sizes[i] != ts[i]) return false;
    return true;
  }
};
static Shape flat(int64_t n) {
  Shape s((at::IntArrayRef()));
  s.numel = n;
  return s;
}
static std::ostream& operator<<(std::ostream& o, const Shape& s) {
  return s.numel >= 0 ? o << s.numel << " elements" : o << "shape " << s.sizes << " (-1: any)";
}

// Pointer to a tensor the binding has just allocated itself.
template <typename T>
static T* fresh(const torch::Tensor& t) {
  return static_cast<T*>(t.data_ptr());
}

// One call of an entry point: the device guard, set to the first tensor's
// device before anything is allocated or launched (engaged only where that is
// not the current device: setting and restoring the current one costs three
// runtime calls per binding call), and the only way from a caller's tensor
// to a kernel pointer.
struct Call {
  const char* who;
  int dev;
  c10::hip::OptionalHIPGuard guard;

  static int device_of(const char* who, const torch::Tensor& first) {
    TORCH_CHECK(first.defined() && first.is_cuda(), who, ": the first tensor must be on the GPU");
    return first.get_device();
  }
  Call(const char* who, const torch::Tensor& first) : who(who), dev(device_of(who, first)) {
    if (dev != c10::hip::current_device()) guard.set_index((c10::DeviceIndex)dev);
  }

  template <typename T, c10::ScalarType ST>
  T* ptr(const torch::Tensor& t, const char* name, const Shape& s) const {
    TORCH_CHECK(t.defined() && t.is_cuda() && t.get_device() == dev,
                who, ": ", name, " must be a tensor on GPU ", dev);
    TORCH_CHECK(t.is_contiguous() && t.scalar_type() == ST && s.fits(t),
                who, ": ", name, " must be contiguous ", ST, " of ", s, ", got ",
                t.scalar_type(), " ", t.sizes(), t.is_contiguous() ? "" : " (strided)");
    return static_cast<T*>(t.data_ptr());
  }
  // Inputs; the _out twins are for buffers of the caller's that a kernel writes.
  const u16* bf16(const torch::Tensor& t, const char* n, const Shape& s) const {
    return ptr<u16, torch::kBFloat16>(t, n, s);
  }
  u16* bf16_out(const torch::Tensor& t, const char* n, const Shape& s) const {
    return ptr<u16, torch::kBFloat16>(t, n, s);
  }
  const float* f32(const torch::Tensor& t, const char* n, const Shape& s) const {
    return ptr<float, torch::kFloat>(t, n, s);
  }
  float* f32_out(const torch::Tensor& t, const char* n, const Shape& s) const {
    return ptr<float, torch::kFloat>(t, n, s);
  }
  const long* i64(const torch::Tensor& t, const char* n, const Shape& s) const {
    return ptr<long, torch::kLong>(t, n, s);
  }
  long* i64_out(const torch::Tensor& t, const char* n, const Shape& s) const {
    return ptr<long, torch::kLong>(t, n, s);
  }
  const int* i32(const torch::Tensor& t, const char* n, const Shape& s) const {
    return ptr<int, torch::kInt>(t, n, s);
  }
  // An optional tensor that is absent is a null pointer.
  const u16* bf16(const c10::optional<torch::Tensor>& t, const char* n, const Shape& s) const {
    return t.has_value() ? bf16(*t, n, s) : nullptr;
  }
  // Size i of a tensor whose rank is already checked, as an int kernel argument.
  int dim(const torch::Tensor& t, int i) const {
    const int64_t n = t.sizes()[i];
    TORCH_CHECK(n <= INT_MAX, who, ": a dimension of ", n, " does not fit int");
    return (int)n;
  }
};

// ---------------------------------------------------------------------------
std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, c10::optional<torch::Tensor> w,
                                       double eps) {
  Call c("rmsnorm_fwd", x);
  const bool fp32 = x.scalar_type() == torch::kFloat;
  const float* xf = fp32 ? c.f32(x, "x", {ANY, ANY}) : nullptr;
  const u16* xb = fp32 ? nullptr : c.bf16(x, "x", {ANY, ANY});
  long N = x.size(0);
  int D = c.dim(x, 1);
  TORCH_CHECK(fp32 || D % 8 == 0, "rmsnorm_fwd: bf16 rows need D % 8 == 0");
  auto y = torch::empty_like(x);
  auto invrms = torch::empty({N}, x.options().dtype(torch::kFloat));
  const float* wp = nullptr;
  torch::Tensor wf;
  if (w.has_value()) {
    wf = w->to(torch::kFloat).contiguous();
    wp = c.f32(wf, "w", flat(D));
  }
  int rows_per_block = 4;  // 256 threads = 4 waves
  long grid = std::min((N + rows_per_block - 1) / rows_per_block, (long)8192);
  if (fp32)
    launch(rmsnorm_fwd_kernel<float, 1>, grid, 256, 0, xf, wp, fresh<float>(y),
           fresh<float>(invrms), N, D, (float)eps);
  else
    launch(rmsnorm_fwd_bf16, grid, 256, 0, xb, wp, fresh<u16>(y), fresh<float>(invrms), N, D,
           (float)eps);
  return {y, invrms};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                       c10::optional<torch::Tensor> w,
                                       torch::Tensor invrms, double eps) {
  Call c("rmsnorm_bwd", dy);
  TORCH_CHECK(!w.has_value(), "rmsnorm_bwd: weighted path unimplemented on HIP "
                              "(the model's norms are weightless)");
  const u16* xp = c.bf16(x, "x", {ANY, ANY});
  long N = x.size(0);
  int D = c.dim(x, 1);
  TORCH_CHECK(D % 8 == 0, "rmsnorm_bwd: D % 8 == 0 required");
  const u16* dyp = c.bf16(dy, "dy", {N, D});
  const float* ip = c.f32(invrms, "invrms", flat(N));
  auto dx = torch::empty_like(x);
  long grid = std::min((N + 3) / 4, (long)8192);
  launch(rmsnorm_bwd_bf16, grid, 256, 0, dyp, xp, ip, fresh<u16>(dx), N, D);
  return {dx, torch::Tensor()};
}

// Fused residual add + RMSNorm (weightless, bf16, D % 8 == 0). Launch
// geometry of rmsnorm_fwd / rmsnorm_bwd: one wave per row, 4 per block.
// f(integral constant): the kernels' template argument for row width D.
template <typename F>
static void dispatch_row_width(int D, F&& f) {
  if (D <= 2048) f(std::integral_constant<int, 4>{});
  else if (D <= 4096) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 0>{});
}

std::vector<torch::Tensor> add_rmsnorm_fwd(torch::Tensor x, torch::Tensor r, double eps) {
  Call c("add_rmsnorm_fwd", x);
  const u16* xp = c.bf16(x, "x", {ANY, ANY});
  const u16* rp = c.bf16(r, "r", x.sizes());
  long N = x.size(0);
  int D = c.dim(x, 1);
  TORCH_CHECK(D % 8 == 0, "add_rmsnorm_fwd: D % 8 == 0 required");
  auto s = torch::empty_like(x);
  auto y = torch::empty_like(x);
  auto invrms = torch::empty({N}, x.options().dtype(torch::kFloat));
  long grid = std::min((N + 3) / 4, (long)8192);
  dispatch_row_width(D, [&](auto w) {
    launch(add_rmsnorm_fwd_bf16<decltype(w)::value>, grid, 256, 0, xp, rp, fresh<u16>(s),
           fresh<u16>(y), fresh<float>(invrms), N, D, (float)eps);
  });
  return {s, y, invrms};
}

torch::Tensor add_rmsnorm_bwd(c10::optional<torch::Tensor> ds, torch::Tensor dy,
                              torch::Tensor s, torch::Tensor invrms) {
  Call c("add_rmsnorm_bwd", dy);
  const u16* sp = c.bf16(s, "s", {ANY, ANY});
  long N = s.size(0);
  int D = c.dim(s, 1);
  TORCH_CHECK(D % 8 == 0, "add_rmsnorm_bwd: D % 8 == 0 required");
  const u16* dyp = c.bf16(dy, "dy", {N, D});
  const u16* dsp = c.bf16(ds, "ds", {N, D});
  const float* ip = c.f32(invrms, "invrms", flat(N));
  auto dx = torch::empty_like(s);
  long grid = std::min((N + 3) / 4, (long)8192);
  dispatch_row_width(D, [&](auto w) {
    launch(add_rmsnorm_bwd_bf16<decltype(w)::value>, grid, 256, 0, dsp, dyp, sp, ip,
           fresh<u16>(dx), N, D);
  });
  return dx;
}

// ---------------------------------------------------------------------------
// What the qkv_prep kernels read besides the gradients, checked once: the
// packed projection (B,T,3,H,C) bf16, LN weights (C,) and RoPE tables of at
// least T rows of C/2, the latter four converted to contiguous fp32.
struct PrepInputs {
  int B, T, H, C;
  const u16* qkv;
  const float *qw, *kw, *sin, *cos;
  torch::Tensor keep[4];  // the fp32 tensors those four point into
};
static PrepInputs prep_inputs(const Call& c, const torch::Tensor& qkv, const torch::Tensor& qw,
                              const torch::Tensor& kw, const torch::Tensor& sin_t,
                              const torch::Tensor& cos_t) {
  PrepInputs in;
  in.qkv = c.bf16(qkv, "qkv", {ANY, ANY, 3, ANY, ANY});
  in.B = c.dim(qkv, 0), in.T = c.dim(qkv, 1), in.H = c.dim(qkv, 3), in.C = c.dim(qkv, 4);
  const int C = in.C;
  // The kernels reduce over C/8 lanes with width-(C/8) shuffles and put
  // 64/(C/8) rows in a wave: C/8 must be a power of two that divides 64.
  TORCH_CHECK(C == 8 || C == 16 || C == 32 || C == 64 || C == 128,
              c.who, ": head dim must be 8, 16, 32, 64 or 128 (got ", C, ")");
  auto fp32 = [&](int slot, const torch::Tensor& t, const char* name, const Shape& s) {
    in.keep[slot] = t.to(torch::kFloat).contiguous();
    return c.f32(in.keep[slot], name, s);
  };
  in.qw = fp32(0, qw, "qw", flat(C));
  in.kw = fp32(1, kw, "kw", flat(C));
  in.sin = fp32(2, sin_t, "sin", {ANY, C / 2});
  in.cos = fp32(3, cos_t, "cos", sin_t.sizes());
  TORCH_CHECK(sin_t.size(0) >= in.T, c.who, ": sin/cos must have at least T rows");
  return in;
}

// SLOTS = 3: q, k and the V copy; SLOTS = 2: q and k only (v undefined).
template <int SLOTS>
static std::vector<torch::Tensor> prep_fwd(const char* who, torch::Tensor qkv, torch::Tensor qw,
                                           torch::Tensor kw, torch::Tensor sin_t,
                                           torch::Tensor cos_t, double eps) {
  Call c(who, qkv);
  const PrepInputs in = prep_inputs(c, qkv, qw, kw, sin_t, cos_t);
  const int B = in.B, T = in.T, H = in.H, C = in.C;
  auto opt = qkv.options();
  auto q = torch::empty({B, H, T, C}, opt);
  auto k = torch::empty({B, H, T, C}, opt);
  torch::Tensor v;
  if (SLOTS == 3) v = torch::empty({B, H, T, C}, opt);
  auto qstats = torch::empty({B, H, T, 2}, opt.dtype(torch::kFloat));
  auto kstats = torch::empty({B, H, T, 2}, opt.dtype(torch::kFloat));
  long nrows = (long)B * T * H * SLOTS;
  long grid = std::min((nrows + 3) / 4, (long)16384);
  launch(qkv_prep_fwd_kernel<SLOTS>, grid, 256, 0, in.qkv, in.qw, in.kw, in.sin, in.cos,
         fresh<u16>(q), fresh<u16>(k), SLOTS == 3 ? fresh<u16>(v) : nullptr,
         fresh<float>(qstats), fresh<float>(kstats), B, T, H, C, (float)eps);
  return {q, k, v, qstats, kstats};
}

// Fills slots 0 and 1 of dqkv, and slot 2 from dv where one is given
// (otherwise attn_bwd_packed writes it). Returns {dqw, dkw}.
static std::vector<torch::Tensor> prep_bwd(const Call& c, torch::Tensor dq, torch::Tensor dk,
                                           const c10::optional<torch::Tensor>& dv,
                                           torch::Tensor qkv, torch::Tensor qw, torch::Tensor kw,
                                           torch::Tensor sin_t, torch::Tensor cos_t,
                                           torch::Tensor qstats, torch::Tensor kstats,
                                           torch::Tensor dqkv) {
  const PrepInputs in = prep_inputs(c, qkv, qw, kw, sin_t, cos_t);
  const int B = in.B, T = in.T, H = in.H, C = in.C;
  const long n = (long)B * H * T * C;
  const u16 *dqp = c.bf16(dq, "dq", flat(n)), *dkp = c.bf16(dk, "dk", flat(n));
  const u16* dvp = c.bf16(dv, "dv", flat(n));
  const float* qsp = c.f32(qstats, "qstats", flat(n / C * 2));
  const float* ksp = c.f32(kstats, "kstats", flat(n / C * 2));
  u16* dqkvp = c.bf16_out(dqkv, "dqkv", qkv.sizes());
  // One row sequence and grid with or without dv (V rows skipped without):
  // that keeps the partial sums, hence dqw and dkw, bit-identical.
  long nrows = (long)B * T * H * 3;
  int nblocks = (int)std::min((nrows + 3) / 4, (long)4096);
  auto dqw_p = torch::empty({nblocks, C}, qkv.options().dtype(torch::kFloat));
  auto dkw_p = torch::empty({nblocks, C}, qkv.options().dtype(torch::kFloat));
  size_t smem = 4 * 2 * C * sizeof(float);  // [waves = 256/64][2][C]
  auto kernel = dvp ? qkv_prep_bwd_kernel<true> : qkv_prep_bwd_kernel<false>;
  launch(kernel, nblocks, 256, smem, dqp, dkp, dvp, in.qkv, in.qw, in.kw, in.sin, in.cos, qsp,
         ksp, dqkvp, fresh<float>(dqw_p), fresh<float>(dkw_p), B, T, H, C);
  return {dqw_p.sum(0).to(qw.scalar_type()), dkw_p.sum(0).to(kw.scalar_type())};
}

std::vector<torch::Tensor> qkv_prep_fwd(torch::Tensor qkv, torch::Tensor qw,
                                        torch::Tensor kw, torch::Tensor sin_t,
                                        torch::Tensor cos_t, double eps) {
  return prep_fwd<3>("qkv_prep_fwd", qkv, qw, kw, sin_t, cos_t, eps);
}

std::vector<torch::Tensor> qkv_prep_bwd(torch::Tensor dq, torch::Tensor dk,
                                        torch::Tensor dv, torch::Tensor qkv,
                                        torch::Tensor qw, torch::Tensor kw,
                                        torch::Tensor sin_t, torch::Tensor cos_t,
                                        torch::Tensor qstats, torch::Tensor kstats,
                                        double eps) {
  Call c("qkv_prep_bwd", dq);
  auto dqkv = torch::empty_like(qkv);
  auto dw = prep_bwd(c, dq, dk, dv, qkv, qw, kw, sin_t, cos_t, qstats, kstats, dqkv);
  return {dqkv, dw[0], dw[1]};
}

// Q/K-only variants: no V copy in either direction.
std::vector<torch::Tensor> qk_prep_fwd(torch::Tensor qkv, torch::Tensor qw,
                                       torch::Tensor kw, torch::Tensor sin_t,
                                       torch::Tensor cos_t, double eps) {
  auto r = prep_fwd<2>("qk_prep_fwd", qkv, qw, kw, sin_t, cos_t, eps);
  return {r[0], r[1], r[3], r[4]};
}

std::vector<torch::Tensor> qk_prep_bwd(torch::Tensor dq, torch::Tensor dk,
                                       torch::Tensor qkv, torch::Tensor qw,
                                       torch::Tensor kw, torch::Tensor sin_t,
                                       torch::Tensor cos_t, torch::Tensor qstats,
                                       torch::Tensor kstats, torch::Tensor dqkv) {
  Call c("qk_prep_bwd", dq);
  return prep_bwd(c, dq, dk, c10::nullopt, qkv, qw, kw, sin_t, cos_t, qstats, kstats, dqkv);
}

// ---------------------------------------------------------------------------
// targets[i] in [0, V) is the caller's contract: checking it would be a sync.
std::vector<torch::Tensor> ce_fwd(torch::Tensor logits, torch::Tensor targets) {
  Call c("ce_fwd", logits);
  const u16* lp = c.bf16(logits, "logits", {ANY, ANY});
  long N = logits.size(0);
  int V = c.dim(logits, 1);
  const long* tp = c.i64(targets, "targets", flat(N));
  auto lse = torch::empty({N}, logits.options().dtype(torch::kFloat));
  auto loss_sum = torch::zeros({1}, logits.options().dtype(torch::kFloat));
  long grid = std::min(N, (long)8192);
  launch(ce_fwd_kernel, grid, 256, 0, lp, tp, fresh<float>(lse), fresh<float>(loss_sum), N, V);
  return {loss_sum.squeeze(0), lse};
}

torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor targets, torch::Tensor lse,
                     torch::Tensor gscale) {
  Call c("ce_bwd", logits);
  const u16* lp = c.bf16(logits, "logits", {ANY, ANY});
  long N = logits.size(0);
  int V = c.dim(logits, 1);
  const long* tp = c.i64(targets, "targets", flat(N));
  const float* lsep = c.f32(lse, "lse", flat(N));
  TORCH_CHECK(gscale.defined() && gscale.numel() == 1, "ce_bwd: gscale must hold one value");
  // gscale = dloss, one value on the device; the kernel wants dloss / N:
  // divide here, without a sync.
  auto gs = (gscale.to(torch::kFloat) / (double)N).contiguous();
  const float* gsp = c.f32(gs, "gscale", flat(1));
  auto dlogits = torch::empty_like(logits);
  long grid = std::min(N, (long)8192);
  launch(ce_bwd_kernel, grid, 256, 0, lp, tp, lsep, gsp, fresh<u16>(dlogits), N, V);
  return dlogits;
}

// ---------------------------------------------------------------------------
void adamw_step(torch::Tensor master, torch::Tensor grad, torch::Tensor m,
                torch::Tensor v, torch::Tensor out_bf16, bool write_bf16,
                torch::Tensor sq_sum, double lr, double b1, double b2, double eps,
                double wd, double grad_scale, double clip_norm, long step) {
  Call c("adamw_step", master);
  long n = master.numel();
  float* mp = c.f32_out(master, "master", flat(n));
  const float* gp = c.f32(grad, "grad", flat(n));
  float *m1 = c.f32_out(m, "m", flat(n)), *m2 = c.f32_out(v, "v", flat(n));
  u16* op = write_bf16 ? c.bf16_out(out_bf16, "out_bf16", flat(n)) : nullptr;
  const float* sqp = c.f32(sq_sum, "sq_sum", flat(1));
  // 1 - beta and the bias corrections in double, rounded once: 1.f - (float)b1
  // is 2 fp32 ulp off 1 - b1 (0.9f is below 0.9 by 2.4e-8, which is 2.4e-7 of
  // 0.1), a bias on every gradient's share of m and v and on mhat/vhat.
  float omb1 = (float)(1.0 - b1), omb2 = (float)(1.0 - b2);
  float bc1 = (float)(1.0 / (1.0 - std::pow(b1, (double)step)));
  float bc2 = (float)(1.0 / (1.0 - std::pow(b2, (double)step)));
  long grid = std::min((n / 4 + 255) / 256 + 1, (long)4096);
  launch(adamw_kernel, grid, 256, 0, mp, gp, m1, m2, op, (int)write_bf16, sqp, (float)lr,
         (float)b1, (float)b2, omb1, omb2, (float)eps, (float)wd, (float)grad_scale,
         (float)clip_norm, bc1, bc2, n);
}

// ---------------------------------------------------------------------------
// Strides (elements) of the three layouts the attention kernels address.
static AttnStrides strides_bhtc(int H, int T, int C) {   // (B,H,T,C)
  return {(long)H * T * C, (long)T * C, C};
}
static AttnStrides strides_bthc(int H, int T, int C) {   // (B,T,H,C)
  return {(long)T * H * C, (long)C, H * C};
}
static AttnStrides strides_qkv_slot(int H, int T, int C) {  // one slot of (B,T,3,H,C)
  return {(long)T * 3 * H * C, (long)C, 3 * H * C};
}

// q and k (B,H,T,C) of every attention entry point, checked. Everything else
// is held to these sizes: {B,H,T,C}, {B,T,H,C}, packed {B,T,3,H,C}, lse B*H*T.
struct AttnQK {
  int B, H, T, C;
  const u16 *q, *k;
  torch::TensorOptions opt;
  long rows() const { return (long)B * H * T; }
};
static AttnQK attn_qk(const Call& c, const torch::Tensor& q, const torch::Tensor& k) {
  const u16* qp = c.bf16(q, "q", {ANY, ANY, ANY, ANY});
  const u16* kp = c.bf16(k, "k", q.sizes());
  TORCH_CHECK(q.size(2) % 128 == 0, "attn: T % 128 == 0 required (got ", q.size(2), ")");
  TORCH_CHECK(q.size(3) == 64 || q.size(3) == 128,
              "attn: head dim 64 or 128 (got ", q.size(3), ")");
  return {c.dim(q, 0), c.dim(q, 1), c.dim(q, 2), c.dim(q, 3), qp, kp, q.options()};
}

// In-kernel dropout (philox.h). Without it the kernels (DROP = false) take
// the neutral values and ignore them.
struct DropArgs {
  uint32_t seed_lo = 0, seed_hi = 0, thr = 0;
  float inv_keep = 1.f;
};
using MaybeDrop = c10::optional<DropArgs>;
static DropArgs drop_args(double p, int64_t seed) {
  TORCH_CHECK(p > 0.0 && p < 1.0, "attn dropout: 0 < p < 1 required (got ", p, ")");
  const uint64_t s = (uint64_t)seed;
  return {(uint32_t)s, (uint32_t)(s >> 32), attn_drop_threshold(p),
          (float)(1.0 / (1.0 - p))};
}
static MaybeDrop drop_if(double p, int64_t seed) {  // p == 0: no dropout
  return p > 0.0 ? MaybeDrop(drop_args(p, seed)) : MaybeDrop();
}

// f(C, NW, DROP) as integral constants, for head dim 64|128 and 4|8 waves.
template <typename F>
static void dispatch_attn(int C, int NW, bool drop, F&& f) {
  dispatch_int<128, 64>(C, [&](auto c) {
    dispatch_int<8, 4>(NW, [&](auto nw) {
      dispatch_flag(drop, [&](auto dr) { f(c, nw, dr); });
    });
  });
}

// One forward launcher for every layout: v is read and o written through
// strides. Measured best: 8-wave workgroups at 2 waves/SIMD with one strip
// per wave, SPW = 1 (the kernels wait on memory, so wave co-residency matters
// most); 4 waves for T % 256 != 0.
// The paired-tile kernel is +4% at C=128 and -4% at C=64: C=128 only.
static void attn_fwd_launch(const AttnQK& a, const u16* vp, AttnStrides sv, u16* op,
                            AttnStrides so, float* lsep, const MaybeDrop& drop) {
  const int B = a.B, H = a.H, T = a.T;
  const int NW = (T % 256 == 0) ? 8 : 4;
  const long grid = (long)B * H * (T / (NW * 32));
  const DropArgs d = drop.value_or(DropArgs{});
  dispatch_attn(a.C, NW, drop.has_value(), [&](auto c, auto nw, auto dr) {
    constexpr int CC = decltype(c)::value, NN = decltype(nw)::value;
    constexpr bool DROP = decltype(dr)::value;
    constexpr bool PAIRED = CC == 128 && NN == 8 && !DROP;
    // K and V^T tiles, double-buffered (two tiles each when paired); the
    // epilogue reuses the region as [NW][32*32] fp32.
    const size_t smem = std::max((size_t)((PAIRED ? 8 : 4) * 32 * CC * 2),
                                 (size_t)(NN * 32 * 32 * 4));
    if constexpr (PAIRED)
      launch(attn_fwd2_kernel<CC, NN>, grid, NN * 64, smem, a.q, a.k, vp, op, lsep,
             B, H, T, sv, so);
    else
      launch(attn_fwd_kernel<CC, NN, 1, DROP>, grid, NN * 64, smem, a.q, a.k, vp, op, lsep,
             B, H, T, sv, so, d.seed_lo, d.seed_hi, d.thr, d.inv_keep);
  });
}

// delta = rowsum(dO * o) over N = B*H*T rows, visited in the memory order of
// dO; do_copy != nullptr: dO is also written there as packed (B,H,T,C).
static void attn_delta_launch(const AttnQK& a, const u16* dop, AttnStrides sdo, const u16* op,
                              AttnStrides so, float* deltap, u16* do_copy) {
  const long N = a.rows();
  TORCH_CHECK(N < (1L << 31), "attn: B*H*T must be below 2^31");
  dispatch_int<128, 64>(a.C, [&](auto c) {  // attn_qk admits these two only
    constexpr int CC = decltype(c)::value;
    constexpr long RPB = 4 * (64 / (CC / 8));  // rows per 4-wave block
    const long dgrid = std::min((N + RPB - 1) / RPB, (long)8192);
    launch(attn_delta_kernel<CC>, dgrid, 256, 0, dop, op, deltap, N, a.H, a.T, sdo, so,
           do_copy, (int)(sdo.h < sdo.r));
  });
}

// One backward launcher for every layout: dO, v, o are read and dv written
// through strides. do_copy: see attn_bwd_packed. Returns {dq, dk} (B,H,T,C).
static std::vector<torch::Tensor> attn_bwd_launch(
    const AttnQK& a, const u16* dop, AttnStrides sdo, const u16* vp, AttnStrides sv,
    const u16* op, AttnStrides so, const float* lsep, u16* dvp, AttnStrides sdv,
    const MaybeDrop& drop, u16* do_copy = nullptr) {
  const int B = a.B, H = a.H, T = a.T, C = a.C;
  auto delta = torch::empty({B, H, T}, a.opt.dtype(torch::kFloat));
  const float* deltap = fresh<float>(delta);
  attn_delta_launch(a, dop, sdo, op, so, fresh<float>(delta), do_copy);
  if (do_copy) {  // the delta kernel left dO as packed (B,H,T,C) there
    dop = do_copy;
    sdo = strides_bhtc(H, T, C);
  }
  auto dq = torch::empty({B, H, T, C}, a.opt);
  auto dk = torch::empty({B, H, T, C}, a.opt);
  // MIDGPT_ATTN_DKV_NW4=1 (read once): 4-wave workgroups for the undropped
  // dkv and dq kernels at every T. Faster at C=64, slower at C=128
  // (profiles/launch_refactor.md).
  static const bool nw4 = getenv("MIDGPT_ATTN_DKV_NW4") != nullptr;
  const int NW = (T % 256 == 0 && !(nw4 && !drop)) ? 8 : 4;
  const long grid = (long)B * H * (T / (NW * 32));
  const DropArgs d = drop.value_or(DropArgs{});
  dispatch_attn(C, NW, drop.has_value(), [&](auto c, auto nw, auto dr) {
    constexpr int CC = decltype(c)::value, NN = decltype(nw)::value;
    constexpr bool DROP = decltype(dr)::value;
    // double-buffered staging: dkv = 2x(Q,Qt,dO,dOt) + lse/delta;
    // dq = 2x(K,V,Kt); both reused as [NW][32*32] fp32. Behind it the
    // resident fragments of the workgroup's own rows (V and a few of K in
    // dkv, dO in dq): [NW][32][C] bf16 for each whole set. Sized so that no
    // instantiation holds fewer workgroups per CU than its registers allow.
    const size_t resident = (size_t)NN * 32 * CC * 2;
    const size_t smem_dkv = (size_t)(2 * 4 * 32 * CC) * 2 + 2 * 64 * 4 +
                            (attn_dkv_vf_lds<CC, NN> ? resident : 0) +
                            (size_t)attn_dkv_kf_lds<CC, NN> * NN * 64 * 16;
    static_assert((size_t)(2 * 4 * 32 * CC) * 2 >= (size_t)NN * 32 * 32 * 4,
                  "epilogue bounce fits");
    const size_t smem_dq = (size_t)(2 * 3 * 32 * CC) * 2 + resident;
    static_assert((size_t)(2 * 3 * 32 * CC) * 2 + (size_t)NN * 32 * CC * 2 >=
                  (size_t)NN * 32 * 32 * 4, "epilogue bounce fits");
    launch(attn_bwd_dkv_kernel<CC, NN, DROP>, grid, NN * 64, smem_dkv, dop, a.q, a.k, vp,
           lsep, deltap, fresh<u16>(dk), dvp, B, H, T, sdo, sv, sdv,
           d.seed_lo, d.seed_hi, d.thr, d.inv_keep);
    launch(attn_bwd_dq_kernel<CC, NN, 1, DROP>, grid, NN * 64, smem_dq, dop, a.q, a.k, vp,
           lsep, deltap, fresh<u16>(dq), B, H, T, sdo, sv,
           d.seed_lo, d.seed_hi, d.thr, d.inv_keep);
  });
  return {dq, dk};
}

// ---------------------------------------------------------------------------
// Entry points, (B,H,T,C) throughout.
static std::vector<torch::Tensor> attn_fwd_bhtc(const char* who, torch::Tensor q,
                                                torch::Tensor k, torch::Tensor v,
                                                const MaybeDrop& drop) {
  Call c(who, q);
  const AttnQK a = attn_qk(c, q, k);
  const u16* vp = c.bf16(v, "v", q.sizes());
  auto o = torch::empty_like(q);
  auto lse = torch::empty({a.B, a.H, a.T}, q.options().dtype(torch::kFloat));
  const AttnStrides st = strides_bhtc(a.H, a.T, a.C);
  attn_fwd_launch(a, vp, st, fresh<u16>(o), st, fresh<float>(lse), drop);
  return {o, lse};
}

static std::vector<torch::Tensor> attn_bwd_bhtc(const char* who, torch::Tensor dO,
                                                torch::Tensor q, torch::Tensor k,
                                                torch::Tensor v, torch::Tensor o,
                                                torch::Tensor lse, const MaybeDrop& drop) {
  Call c(who, dO);
  const AttnQK a = attn_qk(c, q, k);
  const u16 *vp = c.bf16(v, "v", q.sizes()), *op = c.bf16(o, "o", q.sizes());
  const u16* dop = c.bf16(dO, "dO", q.sizes());
  const float* lsep = c.f32(lse, "lse", flat(a.rows()));
  auto dv = torch::empty_like(v);
  const AttnStrides st = strides_bhtc(a.H, a.T, a.C);
  auto r = attn_bwd_launch(a, dop, st, vp, st, op, st, lsep, fresh<u16>(dv), st, drop);
  return {r[0], r[1], dv};
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v) {
  return attn_fwd_bhtc("attn_fwd", q, k, v, MaybeDrop());
}
std::vector<torch::Tensor> attn_bwd(torch::Tensor dO, torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor o, torch::Tensor lse) {
  return attn_bwd_bhtc("attn_bwd", dO, q, k, v, o, lse, MaybeDrop());
}
std::vector<torch::Tensor> attn_fwd_dropout(torch::Tensor q, torch::Tensor k,
                                            torch::Tensor v, double p, int64_t seed) {
  return attn_fwd_bhtc("attn_fwd_dropout", q, k, v, drop_args(p, seed));
}
std::vector<torch::Tensor> attn_bwd_dropout(torch::Tensor dO, torch::Tensor q,
                                            torch::Tensor k, torch::Tensor v,
                                            torch::Tensor o, torch::Tensor lse,
                                            double p, int64_t seed) {
  return attn_bwd_bhtc("attn_bwd_dropout", dO, q, k, v, o, lse, drop_args(p, seed));
}

// ---------------------------------------------------------------------------
// Copy-free layouts around attention: o and dO are (B,T,H,C) (what the output
// projection reads and what its backward hands back) and dV goes straight into
// slot 2 of a caller-supplied (B,T,3,H,C) dqkv. v is either the (B,H,T,C)
// copy or the packed (B,T,3,H,C) projection itself, read in place from slot 2.
// p == 0: no dropout.
static const u16* packed_or_plain_v(const Call& c, const AttnQK& a, const torch::Tensor& v,
                                    AttnStrides* sv) {
  if (v.dim() == 5) {
    *sv = strides_qkv_slot(a.H, a.T, a.C);
    return c.bf16(v, "qkv", {a.B, a.T, 3, a.H, a.C}) + 2L * a.H * a.C;
  }
  *sv = strides_bhtc(a.H, a.T, a.C);
  return c.bf16(v, "v", {a.B, a.H, a.T, a.C});
}

std::vector<torch::Tensor> attn_fwd_packed(torch::Tensor q, torch::Tensor k,
                                           torch::Tensor v, double p, int64_t seed) {
  Call c("attn_fwd_packed", q);
  const AttnQK a = attn_qk(c, q, k);
  AttnStrides sv;
  const u16* vp = packed_or_plain_v(c, a, v, &sv);
  auto o = torch::empty({a.B, a.T, a.H, a.C}, q.options());
  auto lse = torch::empty({a.B, a.H, a.T}, q.options().dtype(torch::kFloat));
  attn_fwd_launch(a, vp, sv, fresh<u16>(o), strides_bthc(a.H, a.T, a.C), fresh<float>(lse),
                  drop_if(p, seed));
  return {o, lse};
}

// stage_do: the delta kernel, which reads dO anyway, also writes it out as
// (B,H,T,C) for the dkv and dq kernels; false: they read (B,T,H,C) in place.
std::vector<torch::Tensor> attn_bwd_packed(torch::Tensor dO, torch::Tensor q,
                                           torch::Tensor k, torch::Tensor v,
                                           torch::Tensor o, torch::Tensor lse,
                                           torch::Tensor dqkv, double p, int64_t seed,
                                           bool stage_do) {
  Call c("attn_bwd_packed", dO);
  const AttnQK a = attn_qk(c, q, k);
  const int B = a.B, H = a.H, T = a.T, C = a.C;
  AttnStrides sv;
  const u16* vp = packed_or_plain_v(c, a, v, &sv);
  u16* dvp = c.bf16_out(dqkv, "dqkv", {B, T, 3, H, C}) + 2L * H * C;
  const u16 *dop = c.bf16(dO, "dO", {B, T, H, C}), *op = c.bf16(o, "o", {B, T, H, C});
  const float* lsep = c.f32(lse, "lse", flat(a.rows()));
  const AttnStrides sdv = strides_qkv_slot(H, T, C), so = strides_bthc(H, T, C);
  torch::Tensor do_copy;
  if (stage_do) do_copy = torch::empty_like(q);
  return attn_bwd_launch(a, dop, so, vp, sv, op, so, lsep, dvp, sdv, drop_if(p, seed),
                         stage_do ? fresh<u16>(do_copy) : nullptr);
}

// The backward's first kernel on its own: delta (B,H,T) of dO and o, which
// are both (B,H,T,C) or, with bthc, both (B,T,H,C); then the packed
// (B,H,T,C) copy of dO that the kernel writes on the way is returned too.
std::vector<torch::Tensor> attn_delta(torch::Tensor dO, torch::Tensor o, bool bthc) {
  Call c("attn_delta", dO);
  const u16* dop = c.bf16(dO, "dO", {ANY, ANY, ANY, ANY});
  const u16* op = c.bf16(o, "o", dO.sizes());
  const int d1 = c.dim(dO, 1), d2 = c.dim(dO, 2), C = c.dim(dO, 3);
  const int H = bthc ? d2 : d1, T = bthc ? d1 : d2;
  TORCH_CHECK(C == 64 || C == 128, "attn_delta: head dim 64 or 128 (got ", C, ")");
  const AttnQK a{c.dim(dO, 0), H, T, C, nullptr, nullptr, dO.options()};
  const AttnStrides st = bthc ? strides_bthc(H, T, C) : strides_bhtc(H, T, C);
  auto delta = torch::empty({a.B, H, T}, dO.options().dtype(torch::kFloat));
  if (!bthc) {
    attn_delta_launch(a, dop, st, op, st, fresh<float>(delta), nullptr);
    return {delta};
  }
  auto do_copy = torch::empty({a.B, H, T, C}, dO.options());
  attn_delta_launch(a, dop, st, op, st, fresh<float>(delta), fresh<u16>(do_copy));
  return {delta, do_copy};
}

// ---------------------------------------------------------------------------
// idx[i] in [0, V) is the caller's contract: checking it would be a sync.
torch::Tensor embedding_bwd(torch::Tensor dy, torch::Tensor idx, long V) {
  Call c("embedding_bwd", dy);
  const u16* dyp = c.bf16(dy, "dy", {ANY, ANY});
  long N = dy.size(0);
  int D = c.dim(dy, 1);
  const long* ip = c.i64(idx, "idx", {N});
  TORCH_CHECK(D % 8 == 0, "embedding_bwd: D % 8 == 0");
  if (D % 64 == 0) {
    // sort-based run-per-wave accumulation (exact fp32, no atomics)
    auto sorted_perm = idx.sort();
    auto sorted = std::get<0>(sorted_perm).contiguous();
    auto perm = std::get<1>(sorted_perm).contiguous();
    auto dw = torch::zeros({V, (long)D}, dy.options());
    const int wpb = 4;  // waves per block
    long grid = (N + wpb - 1) / wpb;
    for (int d0 = 0; d0 < D; d0 += 2048)
      launch(embed_bwd_sorted_kernel, grid, wpb * 64, 0, dyp, fresh<long>(sorted),
             fresh<long>(perm), fresh<u16>(dw), N, D, d0);
    return dw;
  }
  auto dw32 = torch::zeros({V, (long)D}, dy.options().dtype(torch::kFloat));
  long grid = std::min(N, (long)4096);
  launch(embed_bwd_scatter_kernel, grid, 256, 0, dyp, ip, fresh<float>(dw32), N, D);
  auto dw = torch::empty({V, (long)D}, dy.options());
  long n = V * (long)D;
  long cgrid = std::min((n / 4 + 255) / 256 + 1, (long)4096);
  launch(f32_to_bf16_kernel, cgrid, 256, 0, fresh<float>(dw32), fresh<u16>(dw), n);
  return dw;
}

// ---------------------------------------------------------------------------
torch::Tensor gelu_fwd(torch::Tensor x) {
  Call c("gelu_fwd", x);
  long n = x.numel();
  const u16* xp = c.bf16(x, "x", flat(n));
  TORCH_CHECK(n % 8 == 0, "gelu_fwd: numel % 8 == 0 required");
  auto y = torch::empty_like(x);
  long grid = std::min((n / 8 + 255) / 256 + 1, (long)8192);
  launch(gelu_fwd_bf16, grid, 256, 0, xp, fresh<u16>(y), n);
  return y;
}

torch::Tensor gelu_bwd(torch::Tensor dy, torch::Tensor x) {
  Call c("gelu_bwd", dy);
  long n = x.numel();
  const u16 *xp = c.bf16(x, "x", flat(n)), *dyp = c.bf16(dy, "dy", flat(n));
  TORCH_CHECK(n % 8 == 0, "gelu_bwd: numel % 8 == 0 required");
  auto dx = torch::empty_like(x);
  long grid = std::min((n / 8 + 255) / 256 + 1, (long)8192);
  launch(gelu_bwd_bf16, grid, 256, 0, dyp, xp, fresh<u16>(dx), n);
  return dx;
}

// ---------------------------------------------------------------------------
// Batched transpose (transpose.hip): every matrix of the table, one launch.
// table_host (n,5) int64 on the CPU is the truth and is validated here: every
// matrix inside src, every image inside dst, the tile prefix consistent.
// table_dev is its GPU copy, which the kernel reads and the caller keeps
// equal to it (not compared: that would be a sync). max_blocks caps the grid
// (0: enough workgroups to fill the device, the rest by grid-stride).
void transpose_batched(torch::Tensor src, torch::Tensor dst, torch::Tensor table_dev,
                       torch::Tensor table_host, int64_t max_blocks) {
  Call c("transpose_batched", src);
  const int64_t ns = src.numel(), nd = dst.numel();
  const u16* sp = c.bf16(src, "src", flat(ns));
  u16* dp = c.bf16_out(dst, "dst", flat(nd));
  TORCH_CHECK(sp + ns <= dp || dp + nd <= sp, c.who, ": src and dst overlap");
  TORCH_CHECK(!table_host.is_cuda() && table_host.dim() == 2 && table_host.size(1) == TR_COLS &&
              table_host.scalar_type() == torch::kLong && table_host.is_contiguous(),
              c.who, ": the host table must be a contiguous CPU int64 tensor (n, 5)");
  const int64_t n = table_host.size(0);
  TORCH_CHECK(n <= INT_MAX, c.who, ": too many matrices");
  const long* tp = c.i64(table_dev, "table_dev", {n, TR_COLS});
  const int64_t* h = table_host.data_ptr<int64_t>();
  int64_t tiles = 0;
  for (int64_t m = 0; m < n; ++m, h += TR_COLS) {
    const int64_t so = h[0], d_o = h[1], rows = h[2], cols = h[3];
    TORCH_CHECK(rows >= 1 && cols >= 1 && rows <= ns && cols <= ns / rows,
                c.who, ": matrix ", m, " is ", rows, " x ", cols, ", src holds ", ns);
    const int64_t numel = rows * cols;
    TORCH_CHECK(so >= 0 && so <= ns - numel, c.who, ": matrix ", m, " at ", so, " leaves src");
    TORCH_CHECK(d_o >= 0 && numel <= nd && d_o <= nd - numel,
                c.who, ": image ", m, " at ", d_o, " leaves dst");
    TORCH_CHECK(h[4] == tiles, c.who, ": tile prefix of matrix ", m, " is ", h[4],
                ", expected ", tiles);
    tiles += ((rows + TR_TILE - 1) / TR_TILE) * ((cols + TR_TILE - 1) / TR_TILE);
  }
  TORCH_CHECK(max_blocks >= 0, c.who, ": max_blocks must be >= 0");
  const int64_t cap = max_blocks > 0 ? max_blocks : 2048;  // 8 workgroups on each of 256 CUs
  launch(transpose_batched_kernel, (unsigned)std::min(tiles, cap), 256, 0, sp, dp, tp, (int)n,
         (long)tiles);
}

// ---------------------------------------------------------------------------
// KV-cache decode (decode.hip). Caches are (B,H,Tmax,C) bf16, contiguous;
// returns Tmax. pool: the caches are a pool of S >= B slots, (S,H,Tmax,C),
// and *pool receives S.
static int64_t decode_caches(const Call& c, const torch::Tensor& k_cache,
                             const torch::Tensor& v_cache, int B, int H, int C, u16** kp,
                             u16** vp, int* pool = nullptr) {
  TORCH_CHECK(C == 64 || C == 128, c.who, ": head dim 64 or 128 (got ", C, ")");
  *kp = c.bf16_out(k_cache, "k_cache", {pool ? ANY : B, H, ANY, C});
  *vp = c.bf16_out(v_cache, "v_cache", k_cache.sizes());
  if (pool) {
    *pool = c.dim(k_cache, 0);
    TORCH_CHECK(*pool >= B, c.who, ": a pool of ", *pool, " slots cannot hold ", B, " rows");
  }
  return k_cache.size(2);
}

// Host copy of per-sequence positions or lengths: (B,) integers on the CPU.
// The device copy, (B,) int32, is what the kernels read. The two are not
// compared (that would be a sync): keeping them equal is the caller's contract.
static std::vector<int64_t> host_lens(const torch::Tensor& t, int B, const char* who) {
  TORCH_CHECK(!t.is_cuda() && t.dim() == 1 && t.size(0) == B &&
              at::isIntegralType(t.scalar_type(), false),
              who, ": the host copy must be a CPU integer tensor of ", B, " values");
  auto t64 = t.to(torch::kLong).contiguous();
  const int64_t* p = t64.data_ptr<int64_t>();
  return std::vector<int64_t>(p, p + B);
}

// The slot map of a slotted call: batch row b lives in cache slot slots[b].
// Host copy (the truth, validated here: B distinct slots in [0, S); two rows
// in one slot would race on its cache) and the (B,) int32 device copy that
// the kernels read, which the caller keeps equal to it.
struct SlotMap {
  std::vector<int64_t> host;
  const int* dev = nullptr;  // null: not a slotted call
  int S = 0;
};
static SlotMap slot_map(const Call& c, const torch::Tensor& slots_dev,
                        const torch::Tensor& slots_host, int B, int64_t S) {
  SlotMap m;
  m.host = host_lens(slots_host, B, c.who);
  TORCH_CHECK(S <= INT_MAX, c.who, ": too many slots");
  std::vector<bool> seen((size_t)std::max<int64_t>(S, 0), false);
  for (int64_t s : m.host) {
    TORCH_CHECK(s >= 0 && s < S, c.who, ": slot ", s, " is outside the pool of ", S);
    TORCH_CHECK(!seen[(size_t)s], c.who, ": slot ", s, " is named twice");
    seen[(size_t)s] = true;
  }
  m.dev = c.i32(slots_dev, "slots_dev", {B});
  m.S = (int)S;
  return m;
}

// The block table of a paged call: the caches are pools (P,H,PS,C) of P pages
// of PS positions (a power of two in [16, 128]) and position p of batch row b
// lives at row p % PS of page table[b][p / PS]; MP*PS stands where Tmax stands
// elsewhere. Host copy, a CPU integer tensor (B,MP): the truth, validated by
// cover(); the (B,MP) int32 device copy is what the kernels read, and the
// caller keeps the two equal.
struct PageTable {
  torch::Tensor host64;        // keeps `host` alive
  const int64_t* host = nullptr;  // (B, MP), row-major
  const int* dev = nullptr;    // null: not a paged call
  int B = 0, P = 0, MP = 0, PS = 0, shift = 0;
  std::vector<int64_t> written;  // pages that receive writes, over the whole call

  int64_t tmax() const { return (int64_t)MP * PS; }
  // Every entry that covers positions [lo, hi) of row b lies in [0, P); with
  // `write`, no page is named by two of the entries that receive writes (two
  // rows, or two blocks of one row, would race on it): check_writes() after
  // the last row.
  void cover(const Call& c, int b, int64_t lo, int64_t hi, bool write) {
    for (int64_t j = lo / PS; j * PS < hi; ++j) {
      const int64_t pg = host[(size_t)b * MP + j];
      TORCH_CHECK(pg >= 0 && pg < P, c.who, ": block_table[", b, "][", j, "] = ", pg,
                  " is outside the pool of ", P, " pages");
      if (write) written.push_back(pg);
    }
  }
  void check_writes(const Call& c) {
    std::sort(written.begin(), written.end());
    const auto dup = std::adjacent_find(written.begin(), written.end());
    TORCH_CHECK(dup == written.end(), c.who, ": page ", dup == written.end() ? -1 : *dup,
                " receives writes twice");
  }
};
static PageTable page_table(const Call& c, const torch::Tensor& table_dev,
                            const torch::Tensor& table_host, const torch::Tensor& k_pool,
                            const torch::Tensor& v_pool, int B, int H, int C, u16** kp,
                            u16** vp) {
  PageTable t;
  TORCH_CHECK(C == 64 || C == 128, c.who, ": head dim 64 or 128 (got ", C, ")");
  *kp = c.bf16_out(k_pool, "k_pool", {ANY, H, ANY, C});
  *vp = c.bf16_out(v_pool, "v_pool", k_pool.sizes());
  t.B = B;
  t.P = c.dim(k_pool, 0);
  t.PS = c.dim(k_pool, 2);
  TORCH_CHECK(t.PS >= 16 && t.PS <= 128 && (t.PS & (t.PS - 1)) == 0, c.who,
              ": the page size must be a power of two in [16, 128], got ", t.PS);
  while ((1 << t.shift) < t.PS) ++t.shift;
  TORCH_CHECK(!table_host.is_cuda() && table_host.dim() == 2 && table_host.size(0) == B &&
              table_host.size(1) >= 1 && at::isIntegralType(table_host.scalar_type(), false),
              c.who, ": the host block table must be a CPU integer tensor (", B, ", MP)");
  t.MP = c.dim(table_host, 1);
  TORCH_CHECK(t.tmax() <= INT_MAX, c.who, ": MP*PS does not fit int");
  t.host64 = table_host.to(torch::kLong).contiguous();  // no copy for what ops passes
  t.host = t.host64.data_ptr<int64_t>();
  t.dev = c.i32(table_dev, "block_table_dev", {B, t.MP});
  return t;
}

// sin/cos are the FULL tables (rows >= pos+Tn, C/2) fp32; fp32 LN weights are
// used in place, others converted. pos_dev == nullptr: every sequence at
// pos[0]; otherwise sequence b at pos[b] (host) == pos_dev[b] (device).
// slots: sequence b in cache slot slots[b] of a pool (ragged calls only);
// null: in cache row b. table (ragged calls only, not with slots): the caches
// are paged pools and sequence b's rows are found through its block table.
static torch::Tensor kv_append_impl(const Call& c, torch::Tensor qkv, torch::Tensor qw,
                                    torch::Tensor kw, torch::Tensor sin_t, torch::Tensor cos_t,
                                    torch::Tensor k_cache, torch::Tensor v_cache,
                                    const std::vector<int64_t>& pos, const int* pos_dev,
                                    double eps, const torch::Tensor* slots_dev = nullptr,
                                    const torch::Tensor* slots_host = nullptr,
                                    const torch::Tensor* table_dev = nullptr,
                                    const torch::Tensor* table_host = nullptr) {
  const u16* qkvp = c.bf16(qkv, "qkv", {ANY, ANY, 3, ANY, ANY});
  int B = c.dim(qkv, 0), Tn = c.dim(qkv, 1), H = c.dim(qkv, 3), C = c.dim(qkv, 4);
  u16 *kcp, *vcp;
  int S = 0;
  PageTable table;
  if (table_dev) table = page_table(c, *table_dev, *table_host, k_cache, v_cache, B, H, C,
                                    &kcp, &vcp);
  const int64_t Tmax = table_dev ? table.tmax() :
      decode_caches(c, k_cache, v_cache, B, H, C, &kcp, &vcp, slots_dev ? &S : nullptr);
  SlotMap slots;
  if (slots_dev) slots = slot_map(c, *slots_dev, *slots_host, B, S);
  TORCH_CHECK(Tn >= 1, "kv_append: no new tokens");
  TORCH_CHECK(qw.is_contiguous() && kw.is_contiguous(),
              "kv_append: LN weights must be contiguous");
  auto qwf = qw.to(torch::kFloat);
  auto kwf = kw.to(torch::kFloat);
  const float *qwp = c.f32(qwf, "qw", flat(C)), *kwp = c.f32(kwf, "kw", flat(C));
  const float* sinp = c.f32(sin_t, "sin", {ANY, C / 2});
  const float* cosp = c.f32(cos_t, "cos", sin_t.sizes());
  for (int64_t p : pos) {
    TORCH_CHECK(p >= 0 && p + Tn <= Tmax, "kv_append: rows [", p, ", ", p + Tn,
                ") do not fit a cache of ", Tmax, " rows");
    TORCH_CHECK(sin_t.size(0) >= p + Tn, "kv_append: sin/cos tables have ", sin_t.size(0),
                " rows, position ", p + Tn - 1, " needed");
  }
  if (table.dev) {
    for (int b = 0; b < B; ++b) table.cover(c, b, pos[b], pos[b] + Tn, true);
    table.check_writes(c);
  }
  auto q = torch::empty({B, H, Tn, C}, qkv.options());
  const long nrows = (long)B * Tn * H * 3;
  const int rpb = 4 * (WAVE / (C / 8));  // rows per 256-thread block
  const long grid = std::min((nrows + rpb - 1) / rpb, (long)16384);
  dispatch_flag(pos_dev != nullptr, [&](auto ragged) {
    dispatch_flag(slots.dev != nullptr, [&](auto slotted) {
      dispatch_flag(table.dev != nullptr, [&](auto paged) {
        constexpr bool RAGGED = decltype(ragged)::value, SLOTS = decltype(slotted)::value,
                       PAGED = decltype(paged)::value;
        if constexpr ((RAGGED || !SLOTS) && (!PAGED || (RAGGED && !SLOTS)))
          launch(kv_append_kernel<RAGGED, SLOTS, PAGED>, grid, 256, 0, qkvp, qwp, kwp, sinp,
                 cosp, fresh<u16>(q), kcp, vcp, B, Tn, H, C, (long)Tmax, (long)pos[0], pos_dev,
                 (float)eps, slots.dev, slots.S, table.dev, table.P, table.MP, table.shift);
      });
    });
  });
  return q;
}

torch::Tensor kv_append(torch::Tensor qkv, torch::Tensor qw, torch::Tensor kw,
                        torch::Tensor sin_t, torch::Tensor cos_t,
                        torch::Tensor k_cache, torch::Tensor v_cache, int64_t pos,
                        double eps) {
  Call c("kv_append", qkv);
  return kv_append_impl(c, qkv, qw, kw, sin_t, cos_t, k_cache, v_cache, {pos}, nullptr, eps);
}

torch::Tensor kv_append_ragged(torch::Tensor qkv, torch::Tensor qw, torch::Tensor kw,
                               torch::Tensor sin_t, torch::Tensor cos_t,
                               torch::Tensor k_cache, torch::Tensor v_cache,
                               torch::Tensor pos_dev, torch::Tensor pos_host, double eps) {
  Call c("kv_append_ragged", qkv);
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(0) >= 1,
              "kv_append: qkv must be (B,Tn,3,H,C) with B >= 1");
  const int B = c.dim(qkv, 0);
  auto pos = host_lens(pos_host, B, c.who);
  return kv_append_impl(c, qkv, qw, kw, sin_t, cos_t, k_cache, v_cache, pos,
                        c.i32(pos_dev, "pos_dev", {B}), eps);
}

torch::Tensor kv_append_slots(torch::Tensor qkv, torch::Tensor qw, torch::Tensor kw,
                              torch::Tensor sin_t, torch::Tensor cos_t,
                              torch::Tensor k_cache, torch::Tensor v_cache,
                              torch::Tensor pos_dev, torch::Tensor pos_host,
                              torch::Tensor slots_dev, torch::Tensor slots_host, double eps) {
  Call c("kv_append_slots", qkv);
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(0) >= 1,
              "kv_append: qkv must be (B,Tn,3,H,C) with B >= 1");
  const int B = c.dim(qkv, 0);
  auto pos = host_lens(pos_host, B, c.who);
  return kv_append_impl(c, qkv, qw, kw, sin_t, cos_t, k_cache, v_cache, pos,
                        c.i32(pos_dev, "pos_dev", {B}), eps, &slots_dev, &slots_host);
}

torch::Tensor kv_append_paged(torch::Tensor qkv, torch::Tensor qw, torch::Tensor kw,
                              torch::Tensor sin_t, torch::Tensor cos_t,
                              torch::Tensor k_pool, torch::Tensor v_pool,
                              torch::Tensor pos_dev, torch::Tensor pos_host,
                              torch::Tensor table_dev, torch::Tensor table_host, double eps) {
  Call c("kv_append_paged", qkv);
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(0) >= 1,
              "kv_append: qkv must be (B,Tn,3,H,C) with B >= 1");
  const int B = c.dim(qkv, 0);
  auto pos = host_lens(pos_host, B, c.who);
  return kv_append_impl(c, qkv, qw, kw, sin_t, cos_t, k_pool, v_pool, pos,
                        c.i32(pos_dev, "pos_dev", {B}), eps, nullptr, nullptr, &table_dev,
                        &table_host);
}

// Rows [0, lens[b]) of contiguous k, v (B,H,T,C) into the pages that the block
// table names (decode.hip); lens like the positions above: host copy validated,
// (B,) int32 device copy read by the kernel.
void kv_store_paged(torch::Tensor k, torch::Tensor v, torch::Tensor k_pool,
                    torch::Tensor v_pool, torch::Tensor lens_dev, torch::Tensor lens_host,
                    torch::Tensor table_dev, torch::Tensor table_host) {
  Call c("kv_store_paged", k);
  const u16* kp = c.bf16(k, "k", {ANY, ANY, ANY, ANY});
  const u16* vp = c.bf16(v, "v", k.sizes());
  const int B = c.dim(k, 0), H = c.dim(k, 1), T = c.dim(k, 2), C = c.dim(k, 3);
  TORCH_CHECK(B >= 1, c.who, ": k must be (B,H,T,C) with B >= 1");
  u16 *kpp, *vpp;
  PageTable table = page_table(c, table_dev, table_host, k_pool, v_pool, B, H, C, &kpp, &vpp);
  auto lens = host_lens(lens_host, B, c.who);
  const int* lp = c.i32(lens_dev, "lens_dev", {B});
  for (int b = 0; b < B; ++b) {
    TORCH_CHECK(lens[b] >= 0 && lens[b] <= T && lens[b] <= table.tmax(), c.who, ": length ",
                lens[b], " exceeds the ", T, " rows given or the table's ", table.tmax());
    table.cover(c, b, 0, lens[b], true);
  }
  table.check_writes(c);
  const long nunits = (long)B * H * T * (C / 8);
  const long grid = std::min((nunits + 255) / 256, (long)16384);
  launch(kv_store_paged_kernel, grid, 256, 0, kp, vp, kpp, vpp, lp, table.dev, B, H, T, C,
         table.P, table.MP, table.shift);
}

static int decode_cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipGetDeviceProperties(&prop, dev) == hipSuccess)
      cus = prop.multiProcessorCount;
    if (cus <= 0) cus = 256;
  }
  return cus;
}

// num_splits = 0: as many slices as it takes to put DECODE_BLOCKS_PER_CU
// block on every CU, but no slice shorter than DECODE_MIN_SLICE keys. Measured
// (profiles/decode.md): one 256-thread block per CU already keeps ~32 KiB of
// loads in flight there and more slices only add partials traffic; the
// combine launch costs about as much as streaming 300 keys in one block, so
// a range under 2 x 256 keys is not cut at all.
constexpr int DECODE_BLOCKS_PER_CU = 1;
constexpr int DECODE_MIN_SLICE = 256;
constexpr int DECODE_MAX_SPLITS = 64;

int64_t attn_decode_auto_splits(int64_t rows, int64_t kv_len, int64_t cus) {
  const int64_t want = (DECODE_BLOCKS_PER_CU * cus + rows - 1) / rows;
  const int64_t fit = kv_len / DECODE_MIN_SLICE;
  return std::max<int64_t>(1, std::min<int64_t>({want, fit, DECODE_MAX_SPLITS}));
}

// q (B,H,Tq,C): the last Tq of kv_len positions; row i sees keys
// [0, kv_len - Tq + i]. Returns o (B,Tq,H,C). lens_dev == nullptr: every
// sequence has kv_lens[0] positions; otherwise sequence b has kv_lens[b]
// (host) == lens_dev[b] (device), and num_splits = 0 applies the rule to the
// longest. slots as in kv_append_impl.
static torch::Tensor attn_decode_impl(const Call& c, torch::Tensor q, torch::Tensor k_cache,
                                      torch::Tensor v_cache,
                                      const std::vector<int64_t>& kv_lens,
                                      const int* lens_dev, int64_t num_splits,
                                      const torch::Tensor* slots_dev = nullptr,
                                      const torch::Tensor* slots_host = nullptr,
                                      const torch::Tensor* table_dev = nullptr,
                                      const torch::Tensor* table_host = nullptr) {
  const u16* qp = c.bf16(q, "q", {ANY, ANY, ANY, ANY});
  int B = c.dim(q, 0), H = c.dim(q, 1), Tq = c.dim(q, 2), C = c.dim(q, 3);
  u16 *kcp, *vcp;
  int pool = 0;
  PageTable table;
  if (table_dev) table = page_table(c, *table_dev, *table_host, k_cache, v_cache, B, H, C,
                                    &kcp, &vcp);
  const int64_t Tmax = table_dev ? table.tmax() :
      decode_caches(c, k_cache, v_cache, B, H, C, &kcp, &vcp, slots_dev ? &pool : nullptr);
  SlotMap slots;
  if (slots_dev) slots = slot_map(c, *slots_dev, *slots_host, B, pool);
  int64_t kv_max = 0;
  for (int64_t kv_len : kv_lens) {
    TORCH_CHECK(kv_len <= Tmax, "attn_decode: kv_len ", kv_len, " exceeds the cache (", Tmax, ")");
    TORCH_CHECK(Tq >= 1 && Tq <= 16 && Tq <= kv_len,
                "attn_decode: 1 <= Tq <= min(16, kv_len) required (Tq ", Tq, ", kv_len ",
                kv_len, ")");
    kv_max = std::max(kv_max, kv_len);
  }
  if (table.dev)  // reads only: a page may be shared by several rows
    for (int b = 0; b < B; ++b) table.cover(c, b, 0, kv_lens[b], false);
  TORCH_CHECK(num_splits >= 0 && num_splits <= DECODE_MAX_SPLITS,
              "attn_decode: num_splits must be in [0, ", DECODE_MAX_SPLITS, "]");
  const long rows = (long)B * H * Tq;
  TORCH_CHECK(rows > 0 && rows < (1L << 31) && kv_max < (1L << 31),
              "attn_decode: size out of range");
  if (num_splits == 0)
    num_splits = attn_decode_auto_splits(rows, kv_max, decode_cu_count());
  const int S = (int)num_splits;
  auto o = torch::empty({B, Tq, H, C}, q.options());
  torch::Tensor ws_acc, ws_ml;
  float *accp = nullptr, *mlp = nullptr;
  if (S > 1) {
    ws_acc = torch::empty({rows, S, C}, q.options().dtype(torch::kFloat));
    ws_ml = torch::empty({rows, S, 2}, q.options().dtype(torch::kFloat));
    accp = fresh<float>(ws_acc);
    mlp = fresh<float>(ws_ml);
  }
  const float scale = 1.0f / std::sqrt((float)C);
  dispatch_int<128, 64>(C, [&](auto cc) {
    dispatch_flag(lens_dev != nullptr, [&](auto ragged) {
      dispatch_flag(slots.dev != nullptr, [&](auto slotted) {
        dispatch_flag(table.dev != nullptr, [&](auto paged) {
          constexpr bool RAGGED = decltype(ragged)::value, SLOTS = decltype(slotted)::value,
                         PAGED = decltype(paged)::value;
          if constexpr ((RAGGED || !SLOTS) && (!PAGED || (RAGGED && !SLOTS)))
            launch(attn_decode_kernel<decltype(cc)::value, RAGGED, SLOTS, PAGED>, dim3(rows, S),
                   256, 0, qp, kcp, vcp, fresh<u16>(o), accp, mlp, H, Tq, (long)Tmax,
                   (int)kv_lens[0], lens_dev, S, scale, slots.dev, slots.S, table.dev, table.P,
                   table.MP, table.shift);
        });
      });
    });
  });
  if (S > 1)
    launch(attn_decode_combine_kernel, rows, C, 0, accp, mlp, fresh<u16>(o), H, Tq, C, S);
  return o;
}

torch::Tensor attn_decode(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                          int64_t kv_len, int64_t num_splits) {
  Call c("attn_decode", q);
  return attn_decode_impl(c, q, k_cache, v_cache, {kv_len}, nullptr, num_splits);
}

torch::Tensor attn_decode_ragged(torch::Tensor q, torch::Tensor k_cache,
                                 torch::Tensor v_cache, torch::Tensor kv_lens_dev,
                                 torch::Tensor kv_lens_host, int64_t num_splits) {
  Call c("attn_decode_ragged", q);
  TORCH_CHECK(q.dim() == 4 && q.size(0) >= 1, "attn_decode: q must be (B,H,Tq,C) with B >= 1");
  const int B = c.dim(q, 0);
  auto lens = host_lens(kv_lens_host, B, c.who);
  return attn_decode_impl(c, q, k_cache, v_cache, lens,
                          c.i32(kv_lens_dev, "kv_lens_dev", {B}), num_splits);
}

torch::Tensor attn_decode_slots(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                                torch::Tensor kv_lens_dev, torch::Tensor kv_lens_host,
                                torch::Tensor slots_dev, torch::Tensor slots_host,
                                int64_t num_splits) {
  Call c("attn_decode_slots", q);
  TORCH_CHECK(q.dim() == 4 && q.size(0) >= 1, "attn_decode: q must be (B,H,Tq,C) with B >= 1");
  const int B = c.dim(q, 0);
  auto lens = host_lens(kv_lens_host, B, c.who);
  return attn_decode_impl(c, q, k_cache, v_cache, lens,
                          c.i32(kv_lens_dev, "kv_lens_dev", {B}), num_splits, &slots_dev,
                          &slots_host);
}

torch::Tensor attn_decode_paged(torch::Tensor q, torch::Tensor k_pool, torch::Tensor v_pool,
                                torch::Tensor kv_lens_dev, torch::Tensor kv_lens_host,
                                torch::Tensor table_dev, torch::Tensor table_host,
                                int64_t num_splits) {
  Call c("attn_decode_paged", q);
  TORCH_CHECK(q.dim() == 4 && q.size(0) >= 1, "attn_decode: q must be (B,H,Tq,C) with B >= 1");
  const int B = c.dim(q, 0);
  auto lens = host_lens(kv_lens_host, B, c.who);
  return attn_decode_impl(c, q, k_pool, v_pool, lens,
                          c.i32(kv_lens_dev, "kv_lens_dev", {B}), num_splits, nullptr, nullptr,
                          &table_dev, &table_host);
}

// ---------------------------------------------------------------------------
// One token per row of logits (sampling.hip). top_k: 0 or >= V means all.
torch::Tensor sample_tokens(torch::Tensor logits, double inv_t, int64_t top_k, int64_t seed,
                            int64_t step) {
  Call c("sample_tokens", logits);
  const u16* lp = c.bf16(logits, "logits", {ANY, ANY});
  const int B = c.dim(logits, 0), V = c.dim(logits, 1);
  TORCH_CHECK(V >= 1, "sample_tokens: empty rows");
  const float it = (float)inv_t;
  TORCH_CHECK(std::isfinite(inv_t) && std::isfinite(it) && it > 0.f,
              "sample_tokens: inv_t must be finite and > 0, got ", inv_t);
  TORCH_CHECK(top_k >= 0, "sample_tokens: top_k >= 0 required (0: all), got ", top_k);
  TORCH_CHECK(step >= 0 && step <= (int64_t)UINT32_MAX,
              "sample_tokens: step must be in [0, 2^32), got ", step);
  auto out = torch::empty({(long)B}, logits.options().dtype(torch::kLong));
  const bool has_k = top_k >= 1 && top_k < V;
  const uint64_t s = (uint64_t)seed;
  dispatch_flag(has_k, [&](auto hk) {
    launch(sample_tokens_kernel<decltype(hk)::value>, B, SAMPLE_THREADS, 0, lp,
           fresh<long>(out), V, it, has_k ? (int)top_k : 0, (uint32_t)s, (uint32_t)(s >> 32),
           (uint32_t)step);
  });
  return out;
}

// Per-row parameters: row b draws as sample_tokens(X, inv_t[b], top_k[b],
// seeds[b], steps[b]) draws row rows[b] of an X that holds logits[b] there.
// inv_t[b] == 0 marks a greedy row (score = logit, top_k ignored, lowest index
// of the maximum). The five host tensors, (B,) on the CPU, are the truth and
// are validated. The kernel reads params_dev, (B, 6) int32 on the GPU, one
// tensor so that a caller uploads it once for as long as the rows stay:
//   [b] = {seed low word, seed high word, step, row, bits of fp32 inv_t, top_k}
// (top_k clamped to INT_MAX; 0 or >= V: all). It is not compared with the host
// values (that would be a sync): keeping them equal is the caller's contract.
torch::Tensor sample_tokens_rows(torch::Tensor logits, torch::Tensor params_dev,
                                 torch::Tensor inv_t, torch::Tensor top_k, torch::Tensor seeds,
                                 torch::Tensor steps, torch::Tensor rows) {
  Call c("sample_tokens_rows", logits);
  const u16* lp = c.bf16(logits, "logits", {ANY, ANY});
  const int B = c.dim(logits, 0), V = c.dim(logits, 1);
  TORCH_CHECK(V >= 1, "sample_tokens_rows: empty rows");
  TORCH_CHECK(!inv_t.is_cuda() && inv_t.dim() == 1 && inv_t.size(0) == B &&
              inv_t.scalar_type() == torch::kFloat,
              c.who, ": inv_t must be a CPU float32 tensor of ", B, " values");
  auto itc = inv_t.contiguous();
  for (int b = 0; b < B; ++b) {
    const float it = itc.data_ptr<float>()[b];
    TORCH_CHECK(std::isfinite(it) && it >= 0.f, c.who,
                ": inv_t must be finite and > 0, or 0 for a greedy row, got ", it);
  }
  for (int64_t k : host_lens(top_k, B, c.who))
    TORCH_CHECK(k >= 0, c.who, ": top_k >= 0 required (0: all), got ", k);
  host_lens(seeds, B, c.who);  // any 64 bits
  for (int64_t s : host_lens(steps, B, c.who))
    TORCH_CHECK(s >= 0 && s <= (int64_t)UINT32_MAX, c.who, ": step must be in [0, 2^32), got ", s);
  for (int64_t r : host_lens(rows, B, c.who))
    TORCH_CHECK(r >= 0 && r <= (int64_t)UINT32_MAX, c.who, ": row must be in [0, 2^32), got ", r);
  const int* pp = c.i32(params_dev, "params_dev", {B, SAMPLE_ROW_WORDS});
  auto out = torch::empty({(long)B}, logits.options().dtype(torch::kLong));
  launch(sample_tokens_rows_kernel, B, SAMPLE_THREADS, 0, lp, fresh<long>(out), V, pp);
  return out;
}

// ---------------------------------------------------------------------------
// The probe kernels read fixed extents: A (32,16) and B (16,32), M and B (32,32).
torch::Tensor probe_mfma(torch::Tensor A, torch::Tensor B) {
  Call c("probe_mfma", A);
  const float *ap = c.f32(A, "A", {32, 16}), *bp = c.f32(B, "B", {16, 32});
  auto D = torch::zeros({32, 32}, A.options());
  launch(probe_mfma_kernel, 1, 64, 0, ap, bp, fresh<float>(D));
  return D;
}
torch::Tensor probe_pack(torch::Tensor M, torch::Tensor B) {
  Call c("probe_pack", M);
  const float *mp = c.f32(M, "M", {32, 32}), *bp = c.f32(B, "B", {32, 32});
  auto D = torch::zeros({32, 32}, M.options());
  launch(probe_pack_kernel, 1, 64, 0, mp, bp, fresh<float>(D));
  return D;
}
// pack_bf16 against f2b over the n fp32 bit patterns from start on; the three
// counts (probe.hip) are added into `counts`, int64 of 3 on the GPU.
void probe_bf16_pack(torch::Tensor counts, int64_t start, int64_t n) {
  Call c("probe_bf16_pack", counts);
  long* cp = c.i64_out(counts, "counts", {3});
  TORCH_CHECK(start >= 0 && start <= (int64_t)UINT32_MAX && n >= 0 && n <= (1LL << 32),
              "probe_bf16_pack: start in [0, 2^32) and n in [0, 2^32] required, got ", start,
              " and ", n);
  const long grid = std::min((long)((n + 255) / 256), 4096L);
  launch(probe_bf16_pack_kernel, grid, 256, 0, (uint32_t)start, (unsigned long long)n,
         reinterpret_cast<unsigned long long*>(cp));
}

#include "blaslt.inc"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("rmsnorm_fwd", &rmsnorm_fwd);
  mod.def("rmsnorm_bwd", &rmsnorm_bwd);
  mod.def("qkv_prep_fwd", &qkv_prep_fwd);
  mod.def("qkv_prep_bwd", &qkv_prep_bwd);
  mod.def("add_rmsnorm_fwd", &add_rmsnorm_fwd);
  mod.def("add_rmsnorm_bwd", &add_rmsnorm_bwd);
  mod.def("qk_prep_fwd", &qk_prep_fwd);
  mod.def("qk_prep_bwd", &qk_prep_bwd);
  mod.def("ce_fwd", &ce_fwd);
  mod.def("ce_bwd", &ce_bwd);
  mod.def("adamw_step", &adamw_step);
  mod.def("attn_fwd", &attn_fwd);
  mod.def("attn_bwd", &attn_bwd);
  mod.def("attn_delta", &attn_delta, py::arg("dO"), py::arg("o"), py::arg("bthc"));
  mod.def("attn_fwd_dropout", &attn_fwd_dropout);
  mod.def("attn_bwd_dropout", &attn_bwd_dropout);
  mod.def("attn_fwd_packed", &attn_fwd_packed, py::arg("q"), py::arg("k"),
          py::arg("v"), py::arg("p") = 0.0, py::arg("seed") = 0);
  mod.def("attn_bwd_packed", &attn_bwd_packed, py::arg("dO"), py::arg("q"),
          py::arg("k"), py::arg("v"), py::arg("o"), py::arg("lse"),
          py::arg("dqkv"), py::arg("p") = 0.0, py::arg("seed") = 0,
          py::arg("stage_do") = true);
  mod.def("kv_append", &kv_append, py::arg("qkv"), py::arg("qw"), py::arg("kw"),
          py::arg("sin"), py::arg("cos"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("pos"), py::arg("eps") = 1e-6);
  mod.def("attn_decode", &attn_decode, py::arg("q"), py::arg("k_cache"),
          py::arg("v_cache"), py::arg("kv_len"), py::arg("num_splits") = 0);
  mod.def("kv_append_ragged", &kv_append_ragged, py::arg("qkv"), py::arg("qw"),
          py::arg("kw"), py::arg("sin"), py::arg("cos"), py::arg("k_cache"),
          py::arg("v_cache"), py::arg("pos_dev"), py::arg("pos_host"),
          py::arg("eps") = 1e-6);
  mod.def("attn_decode_ragged", &attn_decode_ragged, py::arg("q"), py::arg("k_cache"),
          py::arg("v_cache"), py::arg("kv_lens_dev"), py::arg("kv_lens_host"),
          py::arg("num_splits") = 0);
  mod.def("kv_append_slots", &kv_append_slots, py::arg("qkv"), py::arg("qw"), py::arg("kw"),
          py::arg("sin"), py::arg("cos"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("pos_dev"), py::arg("pos_host"), py::arg("slots_dev"),
          py::arg("slots_host"), py::arg("eps") = 1e-6);
  mod.def("attn_decode_slots", &attn_decode_slots, py::arg("q"), py::arg("k_cache"),
          py::arg("v_cache"), py::arg("kv_lens_dev"), py::arg("kv_lens_host"),
          py::arg("slots_dev"), py::arg("slots_host"), py::arg("num_splits") = 0);
  mod.def("kv_append_paged", &kv_append_paged, py::arg("qkv"), py::arg("qw"), py::arg("kw"),
          py::arg("sin"), py::arg("cos"), py::arg("k_pool"), py::arg("v_pool"),
          py::arg("pos_dev"), py::arg("pos_host"), py::arg("block_table_dev"),
          py::arg("block_table_host"), py::arg("eps") = 1e-6);
  mod.def("attn_decode_paged", &attn_decode_paged, py::arg("q"), py::arg("k_pool"),
          py::arg("v_pool"), py::arg("kv_lens_dev"), py::arg("kv_lens_host"),
          py::arg("block_table_dev"), py::arg("block_table_host"), py::arg("num_splits") = 0);
  mod.def("kv_store_paged", &kv_store_paged, py::arg("k"), py::arg("v"), py::arg("k_pool"),
          py::arg("v_pool"), py::arg("lens_dev"), py::arg("lens_host"),
          py::arg("block_table_dev"), py::arg("block_table_host"));
  mod.def("attn_decode_auto_splits", &attn_decode_auto_splits, py::arg("rows"),
          py::arg("kv_len"), py::arg("cus"));
  mod.def("sample_tokens", &sample_tokens, py::arg("logits"), py::arg("inv_t"),
          py::arg("top_k"), py::arg("seed"), py::arg("step"));
  mod.def("sample_tokens_rows", &sample_tokens_rows, py::arg("logits"), py::arg("params_dev"),
          py::arg("inv_t"), py::arg("top_k"), py::arg("seeds"), py::arg("steps"),
          py::arg("rows"));
  mod.def("embedding_bwd", &embedding_bwd);
  mod.def("gelu_fwd", &gelu_fwd);
  mod.def("gelu_bwd", &gelu_bwd);
  mod.def("transpose_batched", &transpose_batched, py::arg("src"), py::arg("dst"),
          py::arg("table_dev"), py::arg("table_host"), py::arg("max_blocks") = 0);
  mod.def("lt_probe", &lt_probe);
  mod.def("matmul_dgelu", &matmul_dgelu);
  mod.def("probe_mfma", &probe_mfma);
  mod.def("probe_pack", &probe_pack);
  mod.def("probe_bf16_pack", &probe_bf16_pack);
}
