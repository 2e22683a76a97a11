// Python bindings for the midgpt_amd HIP kernel layer (gfx950).
// Included at the end of ext.hip (single TU — kernel definitions visible).
#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include <type_traits>
#include <vector>

#define CHECK_GPU(x) TORCH_CHECK(x.is_cuda() && x.is_contiguous(), #x " must be contiguous GPU tensor")

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

static void launch_check() {
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "HIP launch failed: ", hipGetErrorString(e));
}

// Launch on the current stream. Dynamic LDS above the 64 KiB default cap
// (gfx950 has 160 KiB/CU) needs the attribute raised first.
template <typename... P, typename... A>
static void launch(void (*kernel)(P...), long grid, int block, size_t smem, A... args) {
  if (smem > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), smem, cur_stream(),
                     static_cast<P>(args)...);
  launch_check();
}

// ---------------------------------------------------------------------------
std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, c10::optional<torch::Tensor> w,
                                       double eps) {
  CHECK_GPU(x);
  long N = x.size(0);
  int D = x.size(1);
  auto y = torch::empty_like(x);
  auto invrms = torch::empty({N}, x.options().dtype(torch::kFloat));
  const float* wp = nullptr;
  torch::Tensor wf;
  if (w.has_value()) {
    wf = w->to(torch::kFloat).contiguous();
    wp = wf.data_ptr<float>();
  }
  int rows_per_block = 4;  // 256 threads = 4 waves
  long grid = std::min((N + rows_per_block - 1) / rows_per_block, (long)8192);
  if (x.scalar_type() == torch::kBFloat16 && D % 8 == 0) {
    hipLaunchKernelGGL(rmsnorm_fwd_bf16, dim3(grid), dim3(256), 0, cur_stream(),
                       (const u16*)x.data_ptr(), wp, (u16*)y.data_ptr(),
                       invrms.data_ptr<float>(), N, D, (float)eps);
  } else if (x.scalar_type() == torch::kFloat) {
    hipLaunchKernelGGL((rmsnorm_fwd_kernel<float, 1>), dim3(grid), dim3(256), 0,
                       cur_stream(), x.data_ptr<float>(), wp, y.data_ptr<float>(),
                       invrms.data_ptr<float>(), N, D, (float)eps);
  } else {
    TORCH_CHECK(false, "rmsnorm: unsupported dtype/shape");
  }
  launch_check();
  return {y, invrms};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                       c10::optional<torch::Tensor> w,
                                       torch::Tensor invrms, double eps) {
  CHECK_GPU(dy); CHECK_GPU(x);
  long N = x.size(0);
  int D = x.size(1);
  auto dx = torch::empty_like(x);
  long grid = std::min((N + 3) / 4, (long)8192);
  TORCH_CHECK(!w.has_value(), "rmsnorm_bwd: weighted path unimplemented on HIP "
                              "(the model's norms are weightless)");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && D % 8 == 0,
              "rmsnorm_bwd: bf16 with D%8==0 required");
  hipLaunchKernelGGL(rmsnorm_bwd_bf16, dim3(grid), dim3(256), 0, cur_stream(),
                     (const u16*)dy.data_ptr(), (const u16*)x.data_ptr(),
                     invrms.data_ptr<float>(), (u16*)dx.data_ptr(), N, D);
  launch_check();
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
  CHECK_GPU(x); CHECK_GPU(r);
  TORCH_CHECK(x.dim() == 2 && r.sizes() == x.sizes(), "add_rmsnorm: x, r must be (N, D)");
  long N = x.size(0);
  int D = x.size(1);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              r.scalar_type() == torch::kBFloat16 && D % 8 == 0,
              "add_rmsnorm: bf16 with D%8==0 required");
  auto s = torch::empty_like(x);
  auto y = torch::empty_like(x);
  auto invrms = torch::empty({N}, x.options().dtype(torch::kFloat));
  long grid = std::min((N + 3) / 4, (long)8192);
  if (N > 0)
    dispatch_row_width(D, [&](auto w) {
      launch(add_rmsnorm_fwd_bf16<decltype(w)::value>, grid, 256, 0,
             (const u16*)x.data_ptr(), (const u16*)r.data_ptr(), (u16*)s.data_ptr(),
             (u16*)y.data_ptr(), invrms.data_ptr<float>(), N, D, (float)eps);
    });
  return {s, y, invrms};
}

torch::Tensor add_rmsnorm_bwd(c10::optional<torch::Tensor> ds, torch::Tensor dy,
                              torch::Tensor s, torch::Tensor invrms) {
  CHECK_GPU(dy); CHECK_GPU(s); CHECK_GPU(invrms);
  TORCH_CHECK(s.dim() == 2 && dy.sizes() == s.sizes(), "add_rmsnorm_bwd: dy, s must be (N, D)");
  long N = s.size(0);
  int D = s.size(1);
  TORCH_CHECK(s.scalar_type() == torch::kBFloat16 &&
              dy.scalar_type() == torch::kBFloat16 && D % 8 == 0,
              "add_rmsnorm_bwd: bf16 with D%8==0 required");
  TORCH_CHECK(invrms.scalar_type() == torch::kFloat && invrms.numel() == N,
              "add_rmsnorm_bwd: invrms must be fp32 (N,)");
  const u16* dsp = nullptr;
  if (ds.has_value()) {
    CHECK_GPU((*ds));
    TORCH_CHECK(ds->scalar_type() == torch::kBFloat16 && ds->sizes() == s.sizes(),
                "add_rmsnorm_bwd: ds must be bf16 (N, D)");
    dsp = (const u16*)ds->data_ptr();
  }
  auto dx = torch::empty_like(s);
  long grid = std::min((N + 3) / 4, (long)8192);
  if (N > 0)
    dispatch_row_width(D, [&](auto w) {
      launch(add_rmsnorm_bwd_bf16<decltype(w)::value>, grid, 256, 0, dsp,
             (const u16*)dy.data_ptr(), (const u16*)s.data_ptr(),
             invrms.data_ptr<float>(), (u16*)dx.data_ptr(), N, D);
    });
  return dx;
}

// ---------------------------------------------------------------------------
// What the qkv_prep kernels read besides the gradients, checked once: the
// packed projection (B,T,3,H,C) bf16, LN weights (C,) and RoPE tables of at
// least T rows of C/2, the latter four as contiguous fp32.
struct PrepInputs {
  int B, T, H, C;
  torch::Tensor qw, kw, sin, cos;  // fp32
};
static PrepInputs prep_inputs(const torch::Tensor& qkv, const torch::Tensor& qw,
                              const torch::Tensor& kw, const torch::Tensor& sin_t,
                              const torch::Tensor& cos_t) {
  CHECK_GPU(qkv);
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16, "qkv_prep: qkv must be bf16");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "qkv_prep: qkv must be (B,T,3,H,C)");
  int B = qkv.size(0), T = qkv.size(1), H = qkv.size(3), C = qkv.size(4);
  // The kernels reduce over C/8 lanes with width-(C/8) shuffles and put
  // 64/(C/8) rows in a wave: C/8 must be a power of two that divides 64.
  TORCH_CHECK(C == 8 || C == 16 || C == 32 || C == 64 || C == 128,
              "qkv_prep: head dim must be 8, 16, 32, 64 or 128 (got ", C, ")");
  TORCH_CHECK(qw.is_cuda() && kw.is_cuda() && qw.numel() == C && kw.numel() == C,
              "qkv_prep: weights must be GPU tensors of (C,)");
  TORCH_CHECK(sin_t.is_cuda() && cos_t.is_cuda() && sin_t.dim() == 2 &&
              sin_t.size(0) >= T && sin_t.size(1) == C / 2 &&
              cos_t.sizes() == sin_t.sizes(),
              "qkv_prep: sin/cos must be GPU tensors of (>= T, C/2)");
  auto f32 = [](const torch::Tensor& t) { return t.to(torch::kFloat).contiguous(); };
  return {B, T, H, C, f32(qw), f32(kw), f32(sin_t), f32(cos_t)};
}

// SLOTS = 3: q, k and the V copy; SLOTS = 2: q and k only (v undefined).
template <int SLOTS>
static std::vector<torch::Tensor> prep_fwd(torch::Tensor qkv, torch::Tensor qw,
                                           torch::Tensor kw, torch::Tensor sin_t,
                                           torch::Tensor cos_t, double eps) {
  const PrepInputs in = prep_inputs(qkv, qw, kw, sin_t, cos_t);
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
  if (nrows > 0)
    hipLaunchKernelGGL(qkv_prep_fwd_kernel<SLOTS>, dim3(grid), dim3(256), 0, cur_stream(),
                       (const u16*)qkv.data_ptr(), in.qw.data_ptr<float>(),
                       in.kw.data_ptr<float>(), in.sin.data_ptr<float>(),
                       in.cos.data_ptr<float>(), (u16*)q.data_ptr(), (u16*)k.data_ptr(),
                       SLOTS == 3 ? (u16*)v.data_ptr() : (u16*)nullptr,
                       qstats.data_ptr<float>(), kstats.data_ptr<float>(),
                       B, T, H, C, (float)eps);
  launch_check();
  return {q, k, v, qstats, kstats};
}

// Fills slots 0 and 1 of dqkv, and slot 2 from dv where one is given
// (otherwise attn_bwd_packed writes it). Returns {dqw, dkw}.
static std::vector<torch::Tensor> prep_bwd(torch::Tensor dq, torch::Tensor dk,
                                           const torch::Tensor* dv, torch::Tensor qkv,
                                           torch::Tensor qw, torch::Tensor kw,
                                           torch::Tensor sin_t, torch::Tensor cos_t,
                                           torch::Tensor qstats, torch::Tensor kstats,
                                           torch::Tensor dqkv) {
  const PrepInputs in = prep_inputs(qkv, qw, kw, sin_t, cos_t);
  const int B = in.B, T = in.T, H = in.H, C = in.C;
  const long n = (long)B * H * T * C;
  for (const torch::Tensor* g : std::initializer_list<const torch::Tensor*>{&dq, &dk, dv}) {
    if (!g) continue;
    CHECK_GPU((*g));
    TORCH_CHECK(g->scalar_type() == torch::kBFloat16 && g->numel() == n,
                "qkv_prep_bwd: dq, dk, dv must be bf16 (B,H,T,C)");
  }
  CHECK_GPU(qstats); CHECK_GPU(kstats); CHECK_GPU(dqkv);
  TORCH_CHECK(qstats.scalar_type() == torch::kFloat &&
              kstats.scalar_type() == torch::kFloat &&
              qstats.numel() == (long)B * H * T * 2 && kstats.numel() == qstats.numel(),
              "qkv_prep_bwd: stats must be fp32 (B,H,T,2)");
  TORCH_CHECK(dqkv.scalar_type() == torch::kBFloat16 && dqkv.sizes() == qkv.sizes(),
              "qkv_prep_bwd: dqkv must be bf16 with qkv's shape");
  // One row sequence and grid with or without dv (V rows skipped without):
  // that keeps the partial sums, hence dqw and dkw, bit-identical.
  long nrows = (long)B * T * H * 3;
  int nblocks = (int)std::min((nrows + 3) / 4, (long)4096);
  auto dqw_p = torch::empty({nblocks, C}, qkv.options().dtype(torch::kFloat));
  auto dkw_p = torch::empty({nblocks, C}, qkv.options().dtype(torch::kFloat));
  size_t smem = 4 * 2 * C * sizeof(float);  // [waves = 256/64][2][C]
  auto kernel = dv ? qkv_prep_bwd_kernel<true> : qkv_prep_bwd_kernel<false>;
  if (nrows > 0)
    hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(256), smem, cur_stream(),
                       (const u16*)dq.data_ptr(), (const u16*)dk.data_ptr(),
                       dv ? (const u16*)dv->data_ptr() : (const u16*)nullptr,
                       (const u16*)qkv.data_ptr(), in.qw.data_ptr<float>(),
                       in.kw.data_ptr<float>(), in.sin.data_ptr<float>(),
                       in.cos.data_ptr<float>(), qstats.data_ptr<float>(),
                       kstats.data_ptr<float>(), (u16*)dqkv.data_ptr(),
                       dqw_p.data_ptr<float>(), dkw_p.data_ptr<float>(), B, T, H, C);
  launch_check();
  return {dqw_p.sum(0).to(qw.scalar_type()), dkw_p.sum(0).to(kw.scalar_type())};
}

std::vector<torch::Tensor> qkv_prep_fwd(torch::Tensor qkv, torch::Tensor qw,
                                        torch::Tensor kw, torch::Tensor sin_t,
                                        torch::Tensor cos_t, double eps) {
  return prep_fwd<3>(qkv, qw, kw, sin_t, cos_t, eps);
}

std::vector<torch::Tensor> qkv_prep_bwd(torch::Tensor dq, torch::Tensor dk,
                                        torch::Tensor dv, torch::Tensor qkv,
                                        torch::Tensor qw, torch::Tensor kw,
                                        torch::Tensor sin_t, torch::Tensor cos_t,
                                        torch::Tensor qstats, torch::Tensor kstats,
                                        double eps) {
  auto dqkv = torch::empty_like(qkv);
  auto dw = prep_bwd(dq, dk, &dv, qkv, qw, kw, sin_t, cos_t, qstats, kstats, dqkv);
  return {dqkv, dw[0], dw[1]};
}

// Q/K-only variants: no V copy in either direction.
std::vector<torch::Tensor> qk_prep_fwd(torch::Tensor qkv, torch::Tensor qw,
                                       torch::Tensor kw, torch::Tensor sin_t,
                                       torch::Tensor cos_t, double eps) {
  auto r = prep_fwd<2>(qkv, qw, kw, sin_t, cos_t, eps);
  return {r[0], r[1], r[3], r[4]};
}

std::vector<torch::Tensor> qk_prep_bwd(torch::Tensor dq, torch::Tensor dk,
                                       torch::Tensor qkv, torch::Tensor qw,
                                       torch::Tensor kw, torch::Tensor sin_t,
                                       torch::Tensor cos_t, torch::Tensor qstats,
                                       torch::Tensor kstats, torch::Tensor dqkv) {
  return prep_bwd(dq, dk, nullptr, qkv, qw, kw, sin_t, cos_t, qstats, kstats, dqkv);
}

// ---------------------------------------------------------------------------
std::vector<torch::Tensor> ce_fwd(torch::Tensor logits, torch::Tensor targets) {
  CHECK_GPU(logits); CHECK_GPU(targets);
  TORCH_CHECK(logits.scalar_type() == torch::kBFloat16, "logits must be bf16");
  long N = logits.size(0);
  int V = logits.size(1);
  auto lse = torch::empty({N}, logits.options().dtype(torch::kFloat));
  auto loss_sum = torch::zeros({1}, logits.options().dtype(torch::kFloat));
  long grid = std::min(N, (long)8192);
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                     (const u16*)logits.data_ptr(), targets.data_ptr<long>(),
                     lse.data_ptr<float>(), loss_sum.data_ptr<float>(), N, V);
  launch_check();
  return {loss_sum.squeeze(0), lse};
}

torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor targets, torch::Tensor lse,
                     torch::Tensor gscale) {
  CHECK_GPU(logits);
  long N = logits.size(0);
  int V = logits.size(1);
  auto dlogits = torch::empty_like(logits);
  // gscale tensor = dloss (scalar); kernel multiplies by 1/N itself? no —
  // host passes dloss/N as a device scalar: divide here without sync.
  auto gs = (gscale.to(torch::kFloat) / (double)N).contiguous();
  long grid = std::min(N, (long)8192);
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                     (const u16*)logits.data_ptr(), targets.data_ptr<long>(),
                     lse.data_ptr<float>(), gs.data_ptr<float>(),
                     (u16*)dlogits.data_ptr(), N, V);
  launch_check();
  return dlogits;
}

// ---------------------------------------------------------------------------
void adamw_step(torch::Tensor master, torch::Tensor grad, torch::Tensor m,
                torch::Tensor v, torch::Tensor out_bf16, bool write_bf16,
                torch::Tensor sq_sum, double lr, double b1, double b2, double eps,
                double wd, double grad_scale, double clip_norm, long step) {
  CHECK_GPU(master);
  long n = master.numel();
  float bc1 = 1.f / (1.f - powf((float)b1, (float)step));
  float bc2 = 1.f / (1.f - powf((float)b2, (float)step));
  long grid = std::min((n / 4 + 255) / 256 + 1, (long)4096);
  hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                     master.data_ptr<float>(), grad.data_ptr<float>(),
                     m.data_ptr<float>(), v.data_ptr<float>(),
                     write_bf16 ? (u16*)out_bf16.data_ptr() : nullptr,
                     (int)write_bf16, sq_sum.data_ptr<float>(),
                     (float)lr, (float)b1, (float)b2, (float)eps, (float)wd,
                     (float)grad_scale, (float)clip_norm, bc1, bc2, n);
  launch_check();
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

// Argument checks shared by every attention entry point.
static void check_attn_qk(const torch::Tensor& q, const torch::Tensor& k) {
  CHECK_GPU(q); CHECK_GPU(k);
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
              k.scalar_type() == torch::kBFloat16, "attn: bf16 required");
  TORCH_CHECK(q.dim() == 4 && k.sizes() == q.sizes(), "attn: q, k must be (B,H,T,C)");
  TORCH_CHECK(q.size(2) % 128 == 0, "attn: T % 128 == 0 required (got ", q.size(2), ")");
  TORCH_CHECK(q.size(3) == 64 || q.size(3) == 128,
              "attn: head dim 64 or 128 (got ", q.size(3), ")");
}
static void check_attn_bhtc(const torch::Tensor& q, const torch::Tensor& x,
                            const char* name) {
  CHECK_GPU(x);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.sizes() == q.sizes(),
              "attn: ", name, " must be bf16 (B,H,T,C) like q");
}
// qkv (B,T,3,H,C) that q, k (B,H,T,C) were made from.
static void check_attn_packed(const torch::Tensor& q, const torch::Tensor& qkv,
                              const char* name) {
  CHECK_GPU(qkv);
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16, "attn: ", name, " must be bf16");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(0) == q.size(0) && qkv.size(1) == q.size(2) &&
              qkv.size(2) == 3 && qkv.size(3) == q.size(1) && qkv.size(4) == q.size(3),
              "attn: ", name, " must be (B,T,3,H,C) matching q (B,H,T,C)");
}
static void check_attn_bthc(const torch::Tensor& q, const torch::Tensor& x,
                            const char* name) {
  CHECK_GPU(x);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "attn: ", name, " must be bf16");
  TORCH_CHECK(x.dim() == 4 && x.size(0) == q.size(0) && x.size(1) == q.size(2) &&
              x.size(2) == q.size(1) && x.size(3) == q.size(3),
              "attn: ", name, " must be (B,T,H,C) matching q (B,H,T,C)");
}
static void check_attn_lse(const torch::Tensor& q, const torch::Tensor& lse) {
  CHECK_GPU(lse);
  TORCH_CHECK(lse.scalar_type() == torch::kFloat &&
              lse.numel() == q.size(0) * q.size(1) * q.size(2),
              "attn: lse must be fp32 (B,H,T)");
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
  auto on_drop = [&](auto c, auto nw) {
    if (drop) f(c, nw, std::true_type{});
    else f(c, nw, std::false_type{});
  };
  using c64 = std::integral_constant<int, 64>;
  using c128 = std::integral_constant<int, 128>;
  using w4 = std::integral_constant<int, 4>;
  using w8 = std::integral_constant<int, 8>;
  if (C == 128 && NW == 8) on_drop(c128{}, w8{});
  else if (C == 128) on_drop(c128{}, w4{});
  else if (NW == 8) on_drop(c64{}, w8{});
  else on_drop(c64{}, w4{});
}

// One forward launcher for every layout: v is read and o written through
// strides. Measured best: 8-wave workgroups at 2 waves/SIMD with one strip
// per wave, SPW = 1 (the kernels wait on memory, so wave co-residency matters
// most); 4 waves for T % 256 != 0.
// The paired-tile kernel is +4% at C=128 and -4% at C=64: C=128 only.
static void attn_fwd_launch(torch::Tensor q, torch::Tensor k, const u16* vp,
                            AttnStrides sv, u16* op, AttnStrides so,
                            torch::Tensor lse, const MaybeDrop& drop) {
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  const int NW = (T % 256 == 0) ? 8 : 4;
  const long grid = (long)B * H * (T / (NW * 32));
  const DropArgs d = drop.value_or(DropArgs{});
  const u16 *qp = (const u16*)q.data_ptr(), *kp = (const u16*)k.data_ptr();
  float* lsep = lse.data_ptr<float>();
  dispatch_attn(C, NW, drop.has_value(), [&](auto c, auto nw, auto dr) {
    constexpr int CC = decltype(c)::value, NN = decltype(nw)::value;
    constexpr bool DROP = decltype(dr)::value;
    constexpr bool PAIRED = CC == 128 && NN == 8 && !DROP;
    // K and V^T tiles, double-buffered (two tiles each when paired); the
    // epilogue reuses the region as [NW][32*32] fp32.
    const size_t smem = std::max((size_t)((PAIRED ? 8 : 4) * 32 * CC * 2),
                                 (size_t)(NN * 32 * 32 * 4));
    if constexpr (PAIRED)
      launch(attn_fwd2_kernel<CC, NN>, grid, NN * 64, smem, qp, kp, vp, op, lsep,
             B, H, T, sv, so);
    else
      launch(attn_fwd_kernel<CC, NN, 1, DROP>, grid, NN * 64, smem, qp, kp, vp, op, lsep,
             B, H, T, sv, so, d.seed_lo, d.seed_hi, d.thr, d.inv_keep);
  });
}

// One backward launcher for every layout: dO, v, o are read and dv written
// through strides. do_copy: see attn_bwd_packed. Returns {dq, dk} (B,H,T,C).
static std::vector<torch::Tensor> attn_bwd_launch(
    const u16* dop, AttnStrides sdo, torch::Tensor q, torch::Tensor k,
    const u16* vp, AttnStrides sv, const u16* op, AttnStrides so,
    torch::Tensor lse, u16* dvp, AttnStrides sdv, const MaybeDrop& drop,
    u16* do_copy = nullptr) {
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  long N = (long)B * H * T;
  auto delta = torch::empty({B, H, T}, q.options().dtype(torch::kFloat));
  TORCH_CHECK(N < (1L << 31), "attn: B*H*T must be below 2^31");
  long dgrid = std::min((N + 3) / 4, (long)8192);
  launch(attn_delta_kernel, dgrid, 256, 0, dop, op, delta.data_ptr<float>(), N, C, H, T,
         sdo, so, do_copy, (int)(sdo.h < sdo.r));
  if (do_copy) {  // the delta kernel left dO as packed (B,H,T,C) there
    dop = do_copy;
    sdo = strides_bhtc(H, T, C);
  }
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  // MIDGPT_ATTN_DKV_NW4=1 (read once): 4-wave workgroups for the undropped
  // dkv and dq kernels at every T. Faster at C=64, slower at C=128
  // (profiles/launch_refactor.md).
  static const bool nw4 = getenv("MIDGPT_ATTN_DKV_NW4") != nullptr;
  const int NW = (T % 256 == 0 && !(nw4 && !drop)) ? 8 : 4;
  const long grid = (long)B * H * (T / (NW * 32));
  const DropArgs d = drop.value_or(DropArgs{});
  const u16 *qp = (const u16*)q.data_ptr(), *kp = (const u16*)k.data_ptr();
  const float *lsep = lse.data_ptr<float>(), *deltap = delta.data_ptr<float>();
  dispatch_attn(C, NW, drop.has_value(), [&](auto c, auto nw, auto dr) {
    constexpr int CC = decltype(c)::value, NN = decltype(nw)::value;
    constexpr bool DROP = decltype(dr)::value;
    // double-buffered staging: dkv = 2x(Q,Qt,dO,dOt) + lse/delta;
    // dq = 2x(K,V,Kt) + per-wave dS; both reused as [NW][32*32] fp32.
    const size_t smem_dkv = std::max((size_t)(2 * 4 * 32 * CC) * 2 + 2 * 64 * 4,
                                     (size_t)(NN * 32 * 32 * 4));
    const size_t smem_dq = std::max((size_t)(2 * 3 * 32 * CC) * 2 + NN * 32 * 32 * 2,
                                    (size_t)(NN * 32 * 32 * 4));
    launch(attn_bwd_dkv_kernel<CC, NN, DROP>, grid, NN * 64, smem_dkv, dop, qp, kp, vp,
           lsep, deltap, (u16*)dk.data_ptr(), dvp, B, H, T, sdo, sv, sdv,
           d.seed_lo, d.seed_hi, d.thr, d.inv_keep);
    launch(attn_bwd_dq_kernel<CC, NN, 1, DROP>, grid, NN * 64, smem_dq, dop, qp, kp, vp,
           lsep, deltap, (u16*)dq.data_ptr(), B, H, T, sdo, sv,
           d.seed_lo, d.seed_hi, d.thr, d.inv_keep);
  });
  return {dq, dk};
}

// ---------------------------------------------------------------------------
// Entry points, (B,H,T,C) throughout.
static std::vector<torch::Tensor> attn_fwd_bhtc(torch::Tensor q, torch::Tensor k,
                                                torch::Tensor v, const MaybeDrop& drop) {
  check_attn_qk(q, k);
  check_attn_bhtc(q, v, "v");
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, H, T}, q.options().dtype(torch::kFloat));
  const AttnStrides st = strides_bhtc(H, T, C);
  attn_fwd_launch(q, k, (const u16*)v.data_ptr(), st, (u16*)o.data_ptr(), st, lse, drop);
  return {o, lse};
}

static std::vector<torch::Tensor> attn_bwd_bhtc(torch::Tensor dO, torch::Tensor q,
                                                torch::Tensor k, torch::Tensor v,
                                                torch::Tensor o, torch::Tensor lse,
                                                const MaybeDrop& drop) {
  check_attn_qk(q, k);
  check_attn_bhtc(q, v, "v");
  check_attn_bhtc(q, o, "o");
  check_attn_bhtc(q, dO, "dO");
  check_attn_lse(q, lse);
  int H = q.size(1), T = q.size(2), C = q.size(3);
  auto dv = torch::empty_like(v);
  const AttnStrides st = strides_bhtc(H, T, C);
  auto r = attn_bwd_launch((const u16*)dO.data_ptr(), st, q, k, (const u16*)v.data_ptr(),
                           st, (const u16*)o.data_ptr(), st, lse, (u16*)dv.data_ptr(), st,
                           drop);
  return {r[0], r[1], dv};
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v) {
  return attn_fwd_bhtc(q, k, v, MaybeDrop());
}
std::vector<torch::Tensor> attn_bwd(torch::Tensor dO, torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor o, torch::Tensor lse) {
  return attn_bwd_bhtc(dO, q, k, v, o, lse, MaybeDrop());
}
std::vector<torch::Tensor> attn_fwd_dropout(torch::Tensor q, torch::Tensor k,
                                            torch::Tensor v, double p, int64_t seed) {
  return attn_fwd_bhtc(q, k, v, drop_args(p, seed));
}
std::vector<torch::Tensor> attn_bwd_dropout(torch::Tensor dO, torch::Tensor q,
                                            torch::Tensor k, torch::Tensor v,
                                            torch::Tensor o, torch::Tensor lse,
                                            double p, int64_t seed) {
  return attn_bwd_bhtc(dO, q, k, v, o, lse, drop_args(p, seed));
}

// ---------------------------------------------------------------------------
// Copy-free layouts around attention: o and dO are (B,T,H,C) (what the output
// projection reads and what its backward hands back) and dV goes straight into
// slot 2 of a caller-supplied (B,T,3,H,C) dqkv. v is either the (B,H,T,C)
// copy or the packed (B,T,3,H,C) projection itself, read in place from slot 2.
// p == 0: no dropout.
static const u16* packed_or_plain_v(const torch::Tensor& q, const torch::Tensor& v,
                                    AttnStrides* sv) {
  int H = q.size(1), T = q.size(2), C = q.size(3);
  if (v.dim() == 5) {
    check_attn_packed(q, v, "qkv");
    *sv = strides_qkv_slot(H, T, C);
    return (const u16*)v.data_ptr() + 2L * H * C;
  }
  check_attn_bhtc(q, v, "v");
  *sv = strides_bhtc(H, T, C);
  return (const u16*)v.data_ptr();
}

std::vector<torch::Tensor> attn_fwd_packed(torch::Tensor q, torch::Tensor k,
                                           torch::Tensor v, double p, int64_t seed) {
  check_attn_qk(q, k);
  AttnStrides sv;
  const u16* vp = packed_or_plain_v(q, v, &sv);
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  auto o = torch::empty({B, T, H, C}, q.options());
  auto lse = torch::empty({B, H, T}, q.options().dtype(torch::kFloat));
  attn_fwd_launch(q, k, vp, sv, (u16*)o.data_ptr(), strides_bthc(H, T, C), lse,
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
  check_attn_qk(q, k);
  AttnStrides sv;
  const u16* vp = packed_or_plain_v(q, v, &sv);
  check_attn_packed(q, dqkv, "dqkv");
  check_attn_bthc(q, dO, "dO");
  check_attn_bthc(q, o, "o");
  check_attn_lse(q, lse);
  int H = q.size(1), T = q.size(2), C = q.size(3);
  u16* dvp = (u16*)dqkv.data_ptr() + 2L * H * C;
  const AttnStrides sdv = strides_qkv_slot(H, T, C), so = strides_bthc(H, T, C);
  torch::Tensor do_copy;
  if (stage_do) do_copy = torch::empty_like(q);
  return attn_bwd_launch((const u16*)dO.data_ptr(), so, q, k, vp, sv,
                         (const u16*)o.data_ptr(), so, lse, dvp, sdv, drop_if(p, seed),
                         stage_do ? (u16*)do_copy.data_ptr() : nullptr);
}

// ---------------------------------------------------------------------------
torch::Tensor embedding_bwd(torch::Tensor dy, torch::Tensor idx, long V) {
  CHECK_GPU(dy); CHECK_GPU(idx);
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16, "embedding_bwd: dy bf16");
  TORCH_CHECK(idx.scalar_type() == torch::kLong, "embedding_bwd: idx int64");
  long N = dy.size(0);
  int D = dy.size(1);
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
      hipLaunchKernelGGL(embed_bwd_sorted_kernel, dim3(grid), dim3(wpb * 64),
                         0, cur_stream(), (const u16*)dy.data_ptr(),
                         sorted.data_ptr<long>(), perm.data_ptr<long>(),
                         (u16*)dw.data_ptr(), N, D, d0);
    launch_check();
    return dw;
  }
  auto dw32 = torch::zeros({V, (long)D}, dy.options().dtype(torch::kFloat));
  long grid = std::min(N, (long)4096);
  hipLaunchKernelGGL(embed_bwd_scatter_kernel, dim3(grid), dim3(256), 0,
                     cur_stream(), (const u16*)dy.data_ptr(),
                     idx.data_ptr<long>(), dw32.data_ptr<float>(), N, D);
  launch_check();
  auto dw = torch::empty({V, (long)D}, dy.options());
  long n = V * (long)D;
  long cgrid = std::min((n / 4 + 255) / 256 + 1, (long)4096);
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(cgrid), dim3(256), 0,
                     cur_stream(), dw32.data_ptr<float>(), (u16*)dw.data_ptr(), n);
  launch_check();
  return dw;
}

// ---------------------------------------------------------------------------
torch::Tensor gelu_fwd(torch::Tensor x) {
  CHECK_GPU(x);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.numel() % 8 == 0,
              "gelu: bf16 with numel %% 8 == 0");
  auto y = torch::empty_like(x);
  long n = x.numel();
  long grid = std::min((n / 8 + 255) / 256 + 1, (long)8192);
  hipLaunchKernelGGL(gelu_fwd_bf16, dim3(grid), dim3(256), 0, cur_stream(),
                     (const u16*)x.data_ptr(), (u16*)y.data_ptr(), n);
  launch_check();
  return y;
}

torch::Tensor gelu_bwd(torch::Tensor dy, torch::Tensor x) {
  CHECK_GPU(dy); CHECK_GPU(x);
  auto dx = torch::empty_like(x);
  long n = x.numel();
  long grid = std::min((n / 8 + 255) / 256 + 1, (long)8192);
  hipLaunchKernelGGL(gelu_bwd_bf16, dim3(grid), dim3(256), 0, cur_stream(),
                     (const u16*)dy.data_ptr(), (const u16*)x.data_ptr(),
                     (u16*)dx.data_ptr(), n);
  launch_check();
  return dx;
}

// ---------------------------------------------------------------------------
// KV-cache decode (decode.hip). Caches are (B,H,Tmax,C) bf16, contiguous.
static void check_decode_cache(const torch::Tensor& k_cache, const torch::Tensor& v_cache,
                               int B, int H, int C, const char* who) {
  CHECK_GPU(k_cache); CHECK_GPU(v_cache);
  TORCH_CHECK(k_cache.scalar_type() == torch::kBFloat16 &&
              v_cache.scalar_type() == torch::kBFloat16, who, ": caches must be bf16");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(0) == B && k_cache.size(1) == H &&
              k_cache.size(3) == C && v_cache.sizes() == k_cache.sizes(),
              who, ": caches must both be (B,H,Tmax,C)");
  TORCH_CHECK(C == 64 || C == 128, who, ": head dim 64 or 128 (got ", C, ")");
}

// Host copy of per-sequence positions or lengths: (B,) integers on the CPU.
static std::vector<int64_t> host_lens(const torch::Tensor& t, int B, const char* who) {
  TORCH_CHECK(!t.is_cuda() && t.dim() == 1 && t.size(0) == B &&
              at::isIntegralType(t.scalar_type(), false),
              who, ": the host copy must be a CPU integer tensor of ", B, " values");
  auto t64 = t.to(torch::kLong).contiguous();
  const int64_t* p = t64.data_ptr<int64_t>();
  return std::vector<int64_t>(p, p + B);
}

// Device copy: (B,) int32 on the GPU, what the kernels read. Not compared
// with the host copy (that would be a sync): keeping them equal is the
// caller's contract.
static const int* dev_lens(const torch::Tensor& t, int B, const char* who) {
  CHECK_GPU(t);
  TORCH_CHECK(t.scalar_type() == torch::kInt && t.dim() == 1 && t.size(0) == B,
              who, ": the device copy must be (", B, ",) int32");
  return t.data_ptr<int>();
}

// sin/cos are the FULL tables (rows >= pos+Tn, C/2) fp32; fp32 LN weights are
// used in place, others converted. pos_dev == nullptr: every sequence at
// pos[0]; otherwise sequence b at pos[b] (host) == pos_dev[b] (device).
static torch::Tensor kv_append_impl(torch::Tensor qkv, torch::Tensor qw, torch::Tensor kw,
                                    torch::Tensor sin_t, torch::Tensor cos_t,
                                    torch::Tensor k_cache, torch::Tensor v_cache,
                                    const std::vector<int64_t>& pos, const int* pos_dev,
                                    double eps) {
  CHECK_GPU(qkv); CHECK_GPU(sin_t); CHECK_GPU(cos_t); CHECK_GPU(qw); CHECK_GPU(kw);
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16, "kv_append: qkv must be bf16");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "kv_append: qkv must be (B,Tn,3,H,C)");
  int B = qkv.size(0), Tn = qkv.size(1), H = qkv.size(3), C = qkv.size(4);
  check_decode_cache(k_cache, v_cache, B, H, C, "kv_append");
  const int64_t Tmax = k_cache.size(2);
  TORCH_CHECK(Tn >= 1, "kv_append: no new tokens");
  TORCH_CHECK(qw.numel() == C && kw.numel() == C, "kv_append: LN weights must be (C,)");
  TORCH_CHECK(sin_t.scalar_type() == torch::kFloat && cos_t.scalar_type() == torch::kFloat &&
              sin_t.dim() == 2 && sin_t.size(1) == C / 2 && cos_t.sizes() == sin_t.sizes(),
              "kv_append: sin/cos must be fp32 (rows, C/2)");
  for (int64_t p : pos) {
    TORCH_CHECK(p >= 0 && p + Tn <= Tmax, "kv_append: rows [", p, ", ", p + Tn,
                ") do not fit a cache of ", Tmax, " rows");
    TORCH_CHECK(sin_t.size(0) >= p + Tn, "kv_append: sin/cos tables have ", sin_t.size(0),
                " rows, position ", p + Tn - 1, " needed");
  }
  auto q = torch::empty({B, H, Tn, C}, qkv.options());
  auto qwf = qw.to(torch::kFloat);
  auto kwf = kw.to(torch::kFloat);
  const long nrows = (long)B * Tn * H * 3;
  const int rpb = 4 * (WAVE / (C / 8));  // rows per 256-thread block
  const long grid = std::min((nrows + rpb - 1) / rpb, (long)16384);
#define LAUNCH_APPEND(RAGGED)                                                     \
  hipLaunchKernelGGL(kv_append_kernel<RAGGED>, dim3(grid), dim3(256), 0,          \
                     cur_stream(), (const u16*)qkv.data_ptr(),                    \
                     qwf.data_ptr<float>(), kwf.data_ptr<float>(),                \
                     sin_t.data_ptr<float>(), cos_t.data_ptr<float>(),            \
                     (u16*)q.data_ptr(), (u16*)k_cache.data_ptr(),                \
                     (u16*)v_cache.data_ptr(), B, Tn, H, C, (long)Tmax,           \
                     (long)pos[0], pos_dev, (float)eps)
  if (pos_dev) LAUNCH_APPEND(true);
  else LAUNCH_APPEND(false);
#undef LAUNCH_APPEND
  launch_check();
  return q;
}

torch::Tensor kv_append(torch::Tensor qkv, torch::Tensor qw, torch::Tensor kw,
                        torch::Tensor sin_t, torch::Tensor cos_t,
                        torch::Tensor k_cache, torch::Tensor v_cache, int64_t pos,
                        double eps) {
  return kv_append_impl(qkv, qw, kw, sin_t, cos_t, k_cache, v_cache, {pos}, nullptr, eps);
}

torch::Tensor kv_append_ragged(torch::Tensor qkv, torch::Tensor qw, torch::Tensor kw,
                               torch::Tensor sin_t, torch::Tensor cos_t,
                               torch::Tensor k_cache, torch::Tensor v_cache,
                               torch::Tensor pos_dev, torch::Tensor pos_host, double eps) {
  TORCH_CHECK(qkv.dim() == 5, "kv_append: qkv must be (B,Tn,3,H,C)");
  const int B = qkv.size(0);
  TORCH_CHECK(B >= 1, "kv_append: empty batch");
  auto pos = host_lens(pos_host, B, "kv_append_ragged");
  return kv_append_impl(qkv, qw, kw, sin_t, cos_t, k_cache, v_cache, pos,
                        dev_lens(pos_dev, B, "kv_append_ragged"), eps);
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
// longest.
static torch::Tensor attn_decode_impl(torch::Tensor q, torch::Tensor k_cache,
                                      torch::Tensor v_cache,
                                      const std::vector<int64_t>& kv_lens,
                                      const int* lens_dev, int64_t num_splits) {
  CHECK_GPU(q);
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "attn_decode: q must be bf16");
  TORCH_CHECK(q.dim() == 4, "attn_decode: q must be (B,H,Tq,C)");
  int B = q.size(0), H = q.size(1), Tq = q.size(2), C = q.size(3);
  check_decode_cache(k_cache, v_cache, B, H, C, "attn_decode");
  const int64_t Tmax = k_cache.size(2);
  int64_t kv_max = 0;
  for (int64_t kv_len : kv_lens) {
    TORCH_CHECK(kv_len <= Tmax, "attn_decode: kv_len ", kv_len, " exceeds the cache (", Tmax, ")");
    TORCH_CHECK(Tq >= 1 && Tq <= 16 && Tq <= kv_len,
                "attn_decode: 1 <= Tq <= min(16, kv_len) required (Tq ", Tq, ", kv_len ",
                kv_len, ")");
    kv_max = std::max(kv_max, kv_len);
  }
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
    accp = ws_acc.data_ptr<float>();
    mlp = ws_ml.data_ptr<float>();
  }
  const float scale = 1.0f / std::sqrt((float)C);
#define LAUNCH_DECODE(CC, RAGGED)                                                 \
  hipLaunchKernelGGL((attn_decode_kernel<CC, RAGGED>), dim3(rows, S), dim3(256), 0, \
                     cur_stream(), (const u16*)q.data_ptr(),                      \
                     (const u16*)k_cache.data_ptr(), (const u16*)v_cache.data_ptr(), \
                     (u16*)o.data_ptr(), accp, mlp, H, Tq, (long)Tmax,            \
                     (int)kv_lens[0], lens_dev, S, scale)
  if (C == 128) { if (lens_dev) LAUNCH_DECODE(128, true); else LAUNCH_DECODE(128, false); }
  else { if (lens_dev) LAUNCH_DECODE(64, true); else LAUNCH_DECODE(64, false); }
#undef LAUNCH_DECODE
  launch_check();
  if (S > 1) {
    hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(rows), dim3(C), 0, cur_stream(),
                       accp, mlp, (u16*)o.data_ptr(), H, Tq, C, S);
    launch_check();
  }
  return o;
}

torch::Tensor attn_decode(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                          int64_t kv_len, int64_t num_splits) {
  return attn_decode_impl(q, k_cache, v_cache, {kv_len}, nullptr, num_splits);
}

torch::Tensor attn_decode_ragged(torch::Tensor q, torch::Tensor k_cache,
                                 torch::Tensor v_cache, torch::Tensor kv_lens_dev,
                                 torch::Tensor kv_lens_host, int64_t num_splits) {
  TORCH_CHECK(q.dim() == 4, "attn_decode: q must be (B,H,Tq,C)");
  const int B = q.size(0);
  TORCH_CHECK(B >= 1, "attn_decode: empty batch");
  auto lens = host_lens(kv_lens_host, B, "attn_decode_ragged");
  return attn_decode_impl(q, k_cache, v_cache, lens,
                          dev_lens(kv_lens_dev, B, "attn_decode_ragged"), num_splits);
}

// ---------------------------------------------------------------------------
torch::Tensor probe_mfma(torch::Tensor A, torch::Tensor B) {
  CHECK_GPU(A); CHECK_GPU(B);
  auto D = torch::zeros({32, 32}, A.options());
  hipLaunchKernelGGL(probe_mfma_kernel, dim3(1), dim3(64), 0, cur_stream(),
                     A.data_ptr<float>(), B.data_ptr<float>(), D.data_ptr<float>());
  launch_check();
  return D;
}
torch::Tensor probe_pack(torch::Tensor M, torch::Tensor B) {
  CHECK_GPU(M); CHECK_GPU(B);
  auto D = torch::zeros({32, 32}, M.options());
  hipLaunchKernelGGL(probe_pack_kernel, dim3(1), dim3(64), 0, cur_stream(),
                     M.data_ptr<float>(), B.data_ptr<float>(), D.data_ptr<float>());
  launch_check();
  return D;
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
  mod.def("attn_decode_auto_splits", &attn_decode_auto_splits, py::arg("rows"),
          py::arg("kv_len"), py::arg("cus"));
  mod.def("embedding_bwd", &embedding_bwd);
  mod.def("gelu_fwd", &gelu_fwd);
  mod.def("gelu_bwd", &gelu_bwd);
  mod.def("lt_probe", &lt_probe);
  mod.def("matmul_dgelu", &matmul_dgelu);
  mod.def("probe_mfma", &probe_mfma);
  mod.def("probe_pack", &probe_pack);
}
