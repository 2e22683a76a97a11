// Python bindings for the midgpt_amd HIP kernel layer (gfx950).
// Included at the end of ext.hip (single TU — kernel definitions visible).
#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include <vector>

#define CHECK_GPU(x) TORCH_CHECK(x.is_cuda() && x.is_contiguous(), #x " must be contiguous GPU tensor")

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

static void launch_check() {
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "HIP launch failed: ", hipGetErrorString(e));
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
#define LAUNCH_BY_ROW_WIDTH(KERNEL, ...)                                        \
  do {                                                                          \
    if (D <= 2048)                                                              \
      hipLaunchKernelGGL((KERNEL<4>), dim3(grid), dim3(256), 0, cur_stream(),   \
                         __VA_ARGS__);                                          \
    else if (D <= 4096)                                                         \
      hipLaunchKernelGGL((KERNEL<8>), dim3(grid), dim3(256), 0, cur_stream(),   \
                         __VA_ARGS__);                                          \
    else                                                                        \
      hipLaunchKernelGGL((KERNEL<0>), dim3(grid), dim3(256), 0, cur_stream(),   \
                         __VA_ARGS__);                                          \
  } while (0)

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
    LAUNCH_BY_ROW_WIDTH(add_rmsnorm_fwd_bf16, (const u16*)x.data_ptr(),
                        (const u16*)r.data_ptr(), (u16*)s.data_ptr(),
                        (u16*)y.data_ptr(), invrms.data_ptr<float>(), N, D, (float)eps);
  launch_check();
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
    LAUNCH_BY_ROW_WIDTH(add_rmsnorm_bwd_bf16, dsp, (const u16*)dy.data_ptr(),
                        (const u16*)s.data_ptr(), invrms.data_ptr<float>(),
                        (u16*)dx.data_ptr(), N, D);
  launch_check();
  return dx;
}
#undef LAUNCH_BY_ROW_WIDTH

// ---------------------------------------------------------------------------
// The qkv_prep kernels reduce over C/8 lanes with width-(C/8) shuffles and
// put 64/(C/8) rows in a wave: C/8 must be a power of two that divides 64.
static void check_qkv_head_dim(int C) {
  TORCH_CHECK(C == 8 || C == 16 || C == 32 || C == 64 || C == 128,
              "qkv_prep: head dim must be 8, 16, 32, 64 or 128 (got ", C, ")");
}

std::vector<torch::Tensor> qkv_prep_fwd(torch::Tensor qkv, torch::Tensor qw,
                                        torch::Tensor kw, torch::Tensor sin_t,
                                        torch::Tensor cos_t, double eps) {
  CHECK_GPU(qkv);
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16, "qkv must be bf16");
  int B = qkv.size(0), T = qkv.size(1), H = qkv.size(3), C = qkv.size(4);
  check_qkv_head_dim(C);
  auto opt = qkv.options();
  auto q = torch::empty({B, H, T, C}, opt);
  auto k = torch::empty({B, H, T, C}, opt);
  auto v = torch::empty({B, H, T, C}, opt);
  auto qstats = torch::empty({B, H, T, 2}, opt.dtype(torch::kFloat));
  auto kstats = torch::empty({B, H, T, 2}, opt.dtype(torch::kFloat));
  auto qwf = qw.to(torch::kFloat).contiguous();
  auto kwf = kw.to(torch::kFloat).contiguous();
  auto sf = sin_t.to(torch::kFloat).contiguous();
  auto cf = cos_t.to(torch::kFloat).contiguous();
  long nrows = (long)B * T * H * 3;
  long grid = std::min((nrows + 3) / 4, (long)16384);
  hipLaunchKernelGGL(qkv_prep_fwd_kernel<3>, dim3(grid), dim3(256), 0, cur_stream(),
                     (const u16*)qkv.data_ptr(), qwf.data_ptr<float>(),
                     kwf.data_ptr<float>(), sf.data_ptr<float>(), cf.data_ptr<float>(),
                     (u16*)q.data_ptr(), (u16*)k.data_ptr(), (u16*)v.data_ptr(),
                     qstats.data_ptr<float>(), kstats.data_ptr<float>(),
                     B, T, H, C, (float)eps);
  launch_check();
  return {q, k, v, qstats, kstats};
}

std::vector<torch::Tensor> qkv_prep_bwd(torch::Tensor dq, torch::Tensor dk,
                                        torch::Tensor dv, torch::Tensor qkv,
                                        torch::Tensor qw, torch::Tensor kw,
                                        torch::Tensor sin_t, torch::Tensor cos_t,
                                        torch::Tensor qstats, torch::Tensor kstats,
                                        double eps) {
  CHECK_GPU(dq); CHECK_GPU(dk); CHECK_GPU(dv); CHECK_GPU(qkv);
  CHECK_GPU(qstats); CHECK_GPU(kstats);
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 &&
              dq.scalar_type() == torch::kBFloat16 &&
              dk.scalar_type() == torch::kBFloat16 &&
              dv.scalar_type() == torch::kBFloat16,
              "qkv_prep_bwd: qkv, dq, dk, dv must be bf16");
  TORCH_CHECK(qstats.scalar_type() == torch::kFloat &&
              kstats.scalar_type() == torch::kFloat,
              "qkv_prep_bwd: stats must be fp32");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "qkv_prep_bwd: qkv must be (B,T,3,H,C)");
  int B = qkv.size(0), T = qkv.size(1), H = qkv.size(3), C = qkv.size(4);
  check_qkv_head_dim(C);
  TORCH_CHECK(dq.numel() == (long)B * H * T * C && dk.numel() == dq.numel() &&
              dv.numel() == dq.numel() && qstats.numel() == (long)B * H * T * 2 &&
              kstats.numel() == qstats.numel(),
              "qkv_prep_bwd: dq/dk/dv must be (B,H,T,C) and stats (B,H,T,2)");
  auto dqkv = torch::empty_like(qkv);
  auto qwf = qw.to(torch::kFloat).contiguous();
  auto kwf = kw.to(torch::kFloat).contiguous();
  auto sf = sin_t.to(torch::kFloat).contiguous();
  auto cf = cos_t.to(torch::kFloat).contiguous();
  long nrows = (long)B * T * H * 3;
  int nblocks = (int)std::min((nrows + 3) / 4, (long)4096);
  auto dqw_p = torch::empty({nblocks, C}, qkv.options().dtype(torch::kFloat));
  auto dkw_p = torch::empty({nblocks, C}, qkv.options().dtype(torch::kFloat));
  size_t smem = 4 * 2 * C * sizeof(float);  // [waves = 256/64][2][C]
  hipLaunchKernelGGL(qkv_prep_bwd_kernel<true>, dim3(nblocks), dim3(256), smem, cur_stream(),
                     (const u16*)dq.data_ptr(), (const u16*)dk.data_ptr(),
                     (const u16*)dv.data_ptr(), (const u16*)qkv.data_ptr(),
                     qwf.data_ptr<float>(), kwf.data_ptr<float>(),
                     sf.data_ptr<float>(), cf.data_ptr<float>(),
                     qstats.data_ptr<float>(), kstats.data_ptr<float>(),
                     (u16*)dqkv.data_ptr(), dqw_p.data_ptr<float>(),
                     dkw_p.data_ptr<float>(), B, T, H, C);
  launch_check();
  auto dqw = dqw_p.sum(0).to(qw.scalar_type());
  auto dkw = dkw_p.sum(0).to(kw.scalar_type());
  return {dqkv, dqw, dkw};
}

// Q/K-only variants: no V copy in either direction. The backward fills slots
// 0 and 1 of a caller-supplied dqkv (slot 2 is written by attn_bwd_packed).
std::vector<torch::Tensor> qk_prep_fwd(torch::Tensor qkv, torch::Tensor qw,
                                       torch::Tensor kw, torch::Tensor sin_t,
                                       torch::Tensor cos_t, double eps) {
  CHECK_GPU(qkv);
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16, "qkv must be bf16");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "qk_prep_fwd: qkv must be (B,T,3,H,C)");
  int B = qkv.size(0), T = qkv.size(1), H = qkv.size(3), C = qkv.size(4);
  check_qkv_head_dim(C);
  TORCH_CHECK(qw.numel() == C && kw.numel() == C, "qk_prep_fwd: weights must be (C,)");
  TORCH_CHECK(sin_t.numel() == (long)T * (C / 2) && cos_t.numel() == sin_t.numel(),
              "qk_prep_fwd: sin/cos must be (T, C/2)");
  auto opt = qkv.options();
  auto q = torch::empty({B, H, T, C}, opt);
  auto k = torch::empty({B, H, T, C}, opt);
  auto qstats = torch::empty({B, H, T, 2}, opt.dtype(torch::kFloat));
  auto kstats = torch::empty({B, H, T, 2}, opt.dtype(torch::kFloat));
  auto qwf = qw.to(torch::kFloat).contiguous();
  auto kwf = kw.to(torch::kFloat).contiguous();
  auto sf = sin_t.to(torch::kFloat).contiguous();
  auto cf = cos_t.to(torch::kFloat).contiguous();
  long nrows = (long)B * T * H * 2;
  long grid = std::min((nrows + 3) / 4, (long)16384);
  if (nrows > 0)
    hipLaunchKernelGGL(qkv_prep_fwd_kernel<2>, dim3(grid), dim3(256), 0, cur_stream(),
                       (const u16*)qkv.data_ptr(), qwf.data_ptr<float>(),
                       kwf.data_ptr<float>(), sf.data_ptr<float>(), cf.data_ptr<float>(),
                       (u16*)q.data_ptr(), (u16*)k.data_ptr(), (u16*)nullptr,
                       qstats.data_ptr<float>(), kstats.data_ptr<float>(),
                       B, T, H, C, (float)eps);
  launch_check();
  return {q, k, qstats, kstats};
}

std::vector<torch::Tensor> qk_prep_bwd(torch::Tensor dq, torch::Tensor dk,
                                       torch::Tensor qkv, torch::Tensor qw,
                                       torch::Tensor kw, torch::Tensor sin_t,
                                       torch::Tensor cos_t, torch::Tensor qstats,
                                       torch::Tensor kstats, torch::Tensor dqkv) {
  CHECK_GPU(dq); CHECK_GPU(dk); CHECK_GPU(qkv); CHECK_GPU(dqkv);
  CHECK_GPU(qstats); CHECK_GPU(kstats);
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 &&
              dq.scalar_type() == torch::kBFloat16 &&
              dk.scalar_type() == torch::kBFloat16 &&
              dqkv.scalar_type() == torch::kBFloat16,
              "qk_prep_bwd: qkv, dq, dk, dqkv must be bf16");
  TORCH_CHECK(qstats.scalar_type() == torch::kFloat &&
              kstats.scalar_type() == torch::kFloat,
              "qk_prep_bwd: stats must be fp32");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "qk_prep_bwd: qkv must be (B,T,3,H,C)");
  TORCH_CHECK(dqkv.sizes() == qkv.sizes(), "qk_prep_bwd: dqkv must have qkv's shape");
  int B = qkv.size(0), T = qkv.size(1), H = qkv.size(3), C = qkv.size(4);
  check_qkv_head_dim(C);
  TORCH_CHECK(dq.numel() == (long)B * H * T * C && dk.numel() == dq.numel() &&
              qstats.numel() == (long)B * H * T * 2 &&
              kstats.numel() == qstats.numel(),
              "qk_prep_bwd: dq/dk must be (B,H,T,C) and stats (B,H,T,2)");
  TORCH_CHECK(qw.numel() == C && kw.numel() == C, "qk_prep_bwd: weights must be (C,)");
  TORCH_CHECK(sin_t.numel() == (long)T * (C / 2) && cos_t.numel() == sin_t.numel(),
              "qk_prep_bwd: sin/cos must be (T, C/2)");
  auto qwf = qw.to(torch::kFloat).contiguous();
  auto kwf = kw.to(torch::kFloat).contiguous();
  auto sf = sin_t.to(torch::kFloat).contiguous();
  auto cf = cos_t.to(torch::kFloat).contiguous();
  // Same row sequence and grid as qkv_prep_bwd (V rows skipped): that keeps
  // the partial sums, hence dqw and dkw, bit-identical to it.
  long nrows = (long)B * T * H * 3;
  int nblocks = (int)std::min((nrows + 3) / 4, (long)4096);
  auto dqw_p = torch::empty({nblocks, C}, qkv.options().dtype(torch::kFloat));
  auto dkw_p = torch::empty({nblocks, C}, qkv.options().dtype(torch::kFloat));
  size_t smem = 4 * 2 * C * sizeof(float);  // [waves = 256/64][2][C]
  if (nrows > 0)
    hipLaunchKernelGGL(qkv_prep_bwd_kernel<false>, dim3(nblocks), dim3(256), smem,
                       cur_stream(), (const u16*)dq.data_ptr(), (const u16*)dk.data_ptr(),
                       (const u16*)nullptr, (const u16*)qkv.data_ptr(),
                       qwf.data_ptr<float>(), kwf.data_ptr<float>(),
                       sf.data_ptr<float>(), cf.data_ptr<float>(),
                       qstats.data_ptr<float>(), kstats.data_ptr<float>(),
                       (u16*)dqkv.data_ptr(), dqw_p.data_ptr<float>(),
                       dkw_p.data_ptr<float>(), B, T, H, C);
  launch_check();
  auto dqw = dqw_p.sum(0).to(qw.scalar_type());
  auto dkw = dkw_p.sum(0).to(kw.scalar_type());
  return {dqw, dkw};
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

static void check_attn_qk(const torch::Tensor& q, const torch::Tensor& k) {
  CHECK_GPU(q); CHECK_GPU(k);
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
              k.scalar_type() == torch::kBFloat16, "attn: bf16 required");
  TORCH_CHECK(q.dim() == 4 && k.sizes() == q.sizes(), "attn: q, k must be (B,H,T,C)");
  TORCH_CHECK(q.size(2) % 128 == 0, "attn: T % 128 == 0 required (got ", q.size(2), ")");
  TORCH_CHECK(q.size(3) == 64 || q.size(3) == 128,
              "attn: head dim 64 or 128 (got ", q.size(3), ")");
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

// One launcher for every layout: v is read and o written through strides.
static void attn_fwd_launch(torch::Tensor q, torch::Tensor k, const u16* vp,
                            AttnStrides sv, u16* op, AttnStrides so,
                            torch::Tensor lse) {
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  // Measured best: 8-wave WGs at 2 waves/SIMD, SPW=1. The SPW=2
  // mirrored-strip variant (1 wave/SIMD for C=128) and 3-waves/SIMD were
  // both measured slower — SQ_WAIT is memory-wait dominated, so wave
  // co-residency (TLP) matters most. Fallback to 4 waves for small T.
  const int NW = (T % 256 == 0) ? 8 : 4;
  const int SPW = 1;
  long grid = (long)B * H * (T / (NW * 32 * SPW));
  size_t smem = std::max((size_t)(4 * 32 * C * 2), (size_t)(NW * 32 * 32 * 4));
#define LAUNCH_FWD(CC, NN, SS, MM)                                              \
  hipLaunchKernelGGL((attn_fwd_kernel<CC, NN, SS, MM>), dim3(grid),             \
                     dim3(NN * 64),                                             \
                     smem, cur_stream(), (const u16*)q.data_ptr(),              \
                     (const u16*)k.data_ptr(), vp,        \
                     op, lse.data_ptr<float>(), B, H, T, sv, so)
  // depth-2 prefetch single-tile kernel (4 LDS buffers, loads 2 tiles
  // ahead): opt-in A/B via MIDGPT_ATTN_FWD_D2=1
  static const bool fwd_d2 = getenv("MIDGPT_ATTN_FWD_D2") != nullptr;
  if (fwd_d2 && NW == 8) {
    size_t smem_d2 = std::max((size_t)(8 * 32 * C * 2), (size_t)(NW * 32 * 32 * 4));
    if (C == 128)
      hipLaunchKernelGGL((attn_fwd_d2_kernel<128, 8>), dim3(grid), dim3(512),
                         smem_d2, cur_stream(), (const u16*)q.data_ptr(),
                         (const u16*)k.data_ptr(), vp,
                         op, lse.data_ptr<float>(), B, H, T, sv, so);
    else
      hipLaunchKernelGGL((attn_fwd_d2_kernel<64, 8>), dim3(grid), dim3(512),
                         smem_d2, cur_stream(), (const u16*)q.data_ptr(),
                         (const u16*)k.data_ptr(), vp,
                         op, lse.data_ptr<float>(), B, H, T, sv, so);
    launch_check();
    return;
  }
  // paired-tile kernel (one merged rescale per 64 k): measured +4% at
  // C=128, -4% at C=64 -> default for C=128 only (MIDGPT_ATTN_FWD2=1
  // forces it everywhere, MIDGPT_ATTN_FWD1=1 disables).
  static const bool fwd2_force = getenv("MIDGPT_ATTN_FWD2") != nullptr;
  static const bool fwd1_force = getenv("MIDGPT_ATTN_FWD1") != nullptr;
  const bool fwd2 = !fwd1_force && (fwd2_force || C == 128);
  if (fwd2 && NW == 8) {
    size_t smem2 = std::max((size_t)(8 * 32 * C * 2), (size_t)(NW * 32 * 32 * 4));
#define LAUNCH_FWD2(CC)                                                         \
    do {                                                                        \
      if (smem2 > 64 * 1024)                                                    \
        hipFuncSetAttribute(                                                    \
            reinterpret_cast<const void*>(&attn_fwd2_kernel<CC, 8>),            \
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem2);            \
      hipLaunchKernelGGL((attn_fwd2_kernel<CC, 8>), dim3(grid), dim3(512),      \
                         smem2, cur_stream(), (const u16*)q.data_ptr(),         \
                         (const u16*)k.data_ptr(), vp,    \
                         op, lse.data_ptr<float>(), B, H, T, sv, so);   \
    } while (0)
    if (C == 128) LAUNCH_FWD2(128); else LAUNCH_FWD2(64);
#undef LAUNCH_FWD2
    launch_check();
    return;
  }
  static const bool minw3 = getenv("MIDGPT_ATTN_FWD_MINW3") != nullptr;
  if (C == 128 && NW == 8 && minw3) LAUNCH_FWD(128, 8, 1, 3);
  else if (C == 128 && NW == 8) LAUNCH_FWD(128, 8, 1, 2);
  else if (C == 128) LAUNCH_FWD(128, 4, 1, 2);
  else if (NW == 8 && minw3) LAUNCH_FWD(64, 8, 1, 3);
  else if (NW == 8) LAUNCH_FWD(64, 8, 1, 2);
  else LAUNCH_FWD(64, 4, 1, 2);
#undef LAUNCH_FWD
  launch_check();
  return;
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v) {
  CHECK_GPU(q); CHECK_GPU(k); CHECK_GPU(v);
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "attn: bf16 required");
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  TORCH_CHECK(T % 128 == 0, "attn: T % 128 == 0 required (got ", T, ")");
  TORCH_CHECK(C == 64 || C == 128, "attn: head dim 64 or 128 (got ", C, ")");
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, H, T}, q.options().dtype(torch::kFloat));
  const AttnStrides st = strides_bhtc(H, T, C);
  attn_fwd_launch(q, k, (const u16*)v.data_ptr(), st, (u16*)o.data_ptr(), st, lse);
  return {o, lse};
}

// One launcher for every layout: dO, v, o are read and dv written through
// strides. Returns {dq, dk} (packed (B,H,T,C)).
static std::vector<torch::Tensor> attn_bwd_launch(
    const u16* dop, AttnStrides sdo, torch::Tensor q, torch::Tensor k,
    const u16* vp, AttnStrides sv, const u16* op, AttnStrides so,
    torch::Tensor lse, u16* dvp, AttnStrides sdv, u16* do_copy = nullptr) {
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  long N = (long)B * H * T;
  auto delta = torch::empty({B, H, T}, q.options().dtype(torch::kFloat));
  TORCH_CHECK(N < (1L << 31), "attn: B*H*T must be below 2^31");
  long dgrid = std::min((N + 3) / 4, (long)8192);
  hipLaunchKernelGGL(attn_delta_kernel, dim3(dgrid), dim3(256), 0, cur_stream(),
                     dop, op,
                     delta.data_ptr<float>(), N, C, H, T, sdo, so, do_copy,
                     (int)(sdo.h < sdo.r));
  launch_check();
  if (do_copy) {  // the delta kernel left dO as packed (B,H,T,C) there
    dop = do_copy;
    sdo = strides_bhtc(H, T, C);
  }
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  static const bool dkv4 = getenv("MIDGPT_ATTN_DKV_NW4") != nullptr;
  const int NW_A = dkv4 ? 4 : ((T % 256 == 0) ? 8 : 4);  // dkv geometry
  const int NW_B = NW_A;                     // dq geometry
  const int SPW = 1;
  long grid_a = (long)B * H * (T / (NW_A * 32));
  long grid_b = (long)B * H * (T / (NW_B * 32 * SPW));
  // double-buffered staging: dkv = 2x(Q,Qt,dO,dOt) + lse/delta;
  // dq = 2x(K,V,Kt) + per-wave dS. Above the 64 KiB default dynamic-LDS
  // cap (gfx950 has 160 KiB/CU) -> raise the attribute.
  size_t smem_a = std::max((size_t)(2 * 4 * 32 * C) * 2 + 2 * 64 * 4,
                           (size_t)(NW_A * 32 * 32 * 4));
  size_t smem_b = std::max((size_t)(2 * 3 * 32 * C) * 2 + NW_B * 32 * 32 * 2,
                           (size_t)(NW_B * 32 * 32 * 4));
#define LAUNCH_BWD(CC, NA, NB, SS, MM)                                          \
  do {                                                                          \
    if (smem_a > 64 * 1024)                                                     \
      hipFuncSetAttribute(                                                      \
          reinterpret_cast<const void*>(&attn_bwd_dkv_kernel<CC, NA, 0>),       \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_a);             \
    if (smem_b > 64 * 1024)                                                     \
      hipFuncSetAttribute(                                                      \
          reinterpret_cast<const void*>(&attn_bwd_dq_kernel<CC, NB, SS, MM>),   \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_b);             \
    static const char* abl = getenv("MIDGPT_DKV_ABLATE");                      \
    if (abl && abl[0] == '1')                                                   \
      hipLaunchKernelGGL((attn_bwd_dkv_kernel<CC, NA, 1>), dim3(grid_a),        \
                         dim3(NA * 64), smem_a, cur_stream(),                   \
                         dop, (const u16*)q.data_ptr(),   \
                         (const u16*)k.data_ptr(), vp,    \
                         lse.data_ptr<float>(), delta.data_ptr<float>(),        \
                         (u16*)dk.data_ptr(), dvp, B, H, T, sdo, sv, sdv);    \
    else if (abl && abl[0] == '3')                                              \
      hipLaunchKernelGGL((attn_bwd_dkv_kernel<CC, NA, 3>), dim3(grid_a),        \
                         dim3(NA * 64), smem_a, cur_stream(),                   \
                         dop, (const u16*)q.data_ptr(),   \
                         (const u16*)k.data_ptr(), vp,    \
                         lse.data_ptr<float>(), delta.data_ptr<float>(),        \
                         (u16*)dk.data_ptr(), dvp, B, H, T, sdo, sv, sdv);    \
    else if (abl && abl[0] == '4')                                              \
      hipLaunchKernelGGL((attn_bwd_dkv_kernel<CC, NA, 4>), dim3(grid_a),        \
                         dim3(NA * 64), smem_a, cur_stream(),                   \
                         dop, (const u16*)q.data_ptr(),   \
                         (const u16*)k.data_ptr(), vp,    \
                         lse.data_ptr<float>(), delta.data_ptr<float>(),        \
                         (u16*)dk.data_ptr(), dvp, B, H, T, sdo, sv, sdv);    \
    else if (abl && abl[0] == '5')                                              \
      hipLaunchKernelGGL((attn_bwd_dkv_kernel<CC, NA, 5>), dim3(grid_a),        \
                         dim3(NA * 64), smem_a, cur_stream(),                   \
                         dop, (const u16*)q.data_ptr(),   \
                         (const u16*)k.data_ptr(), vp,    \
                         lse.data_ptr<float>(), delta.data_ptr<float>(),        \
                         (u16*)dk.data_ptr(), dvp, B, H, T, sdo, sv, sdv);    \
    else if (abl && abl[0] == '2')                                              \
      hipLaunchKernelGGL((attn_bwd_dkv_kernel<CC, NA, 2>), dim3(grid_a),        \
                         dim3(NA * 64), smem_a, cur_stream(),                   \
                         dop, (const u16*)q.data_ptr(),   \
                         (const u16*)k.data_ptr(), vp,    \
                         lse.data_ptr<float>(), delta.data_ptr<float>(),        \
                         (u16*)dk.data_ptr(), dvp, B, H, T, sdo, sv, sdv);    \
    else                                                                        \
      hipLaunchKernelGGL((attn_bwd_dkv_kernel<CC, NA, 0>), dim3(grid_a),        \
                         dim3(NA * 64), smem_a, cur_stream(),                   \
                         dop, (const u16*)q.data_ptr(),   \
                         (const u16*)k.data_ptr(), vp,    \
                         lse.data_ptr<float>(), delta.data_ptr<float>(),        \
                         (u16*)dk.data_ptr(), dvp, B, H, T, sdo, sv, sdv);    \
    hipLaunchKernelGGL((attn_bwd_dq_kernel<CC, NB, SS, MM>), dim3(grid_b),      \
                       dim3(NB * 64),                                           \
                       smem_b, cur_stream(), dop,         \
                       (const u16*)q.data_ptr(), (const u16*)k.data_ptr(),      \
                       vp, lse.data_ptr<float>(),         \
                       delta.data_ptr<float>(), (u16*)dq.data_ptr(), B, H, T, sdo, sv);  \
  } while (0)
  static const bool bwd_minw3 = getenv("MIDGPT_ATTN_BWD_MINW3") != nullptr;
  if (C == 64 && NW_A == 8 && bwd_minw3 && !getenv("MIDGPT_DKV_ABLATE")) {
    // squeeze to 3 waves/SIMD (K frags re-read from L2; compiler caps
    // VGPRs at 168) — A/B experiment for the 124M config
    if (smem_a > 64 * 1024)
      hipFuncSetAttribute(
          reinterpret_cast<const void*>(&attn_bwd_dkv_kernel<64, 8, 0, 3>),
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_a);
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<64, 8, 0, 3>), dim3(grid_a),
                       dim3(512), smem_a, cur_stream(),
                       dop, (const u16*)q.data_ptr(),
                       (const u16*)k.data_ptr(), vp,
                       lse.data_ptr<float>(), delta.data_ptr<float>(),
                       (u16*)dk.data_ptr(), dvp, B, H, T, sdo, sv, sdv);
    hipLaunchKernelGGL((attn_bwd_dq_kernel<64, 8, 1, 3>), dim3(grid_b),
                       dim3(512), smem_b, cur_stream(),
                       dop, (const u16*)q.data_ptr(),
                       (const u16*)k.data_ptr(), vp,
                       lse.data_ptr<float>(), delta.data_ptr<float>(),
                       (u16*)dq.data_ptr(), B, H, T, sdo, sv);
    launch_check();
    return {dq, dk};
  }
  if (C == 128 && NW_A == 8) LAUNCH_BWD(128, 8, 8, 1, 2);
  else if (C == 128) LAUNCH_BWD(128, 4, 4, 1, 2);
  else if (NW_B == 8) LAUNCH_BWD(64, 8, 8, 1, 2);
  else LAUNCH_BWD(64, 4, 4, 1, 2);
#undef LAUNCH_BWD
  launch_check();
  return {dq, dk};
}

std::vector<torch::Tensor> attn_bwd(torch::Tensor dO, torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor o, torch::Tensor lse) {
  CHECK_GPU(dO); CHECK_GPU(q);
  int H = q.size(1), T = q.size(2), C = q.size(3);
  auto dv = torch::empty_like(v);
  const AttnStrides st = strides_bhtc(H, T, C);
  auto r = attn_bwd_launch((const u16*)dO.data_ptr(), st, q, k,
                           (const u16*)v.data_ptr(), st, (const u16*)o.data_ptr(), st,
                           lse, (u16*)dv.data_ptr(), st);
  return {r[0], r[1], dv};
}

// ---------------------------------------------------------------------------
// Attention with in-kernel dropout (philox.h). Fixed dispatch: the SPW=1,
// 2-waves/SIMD single-tile kernels with DROP=true, NW from T as above; none
// of the experiment environment switches apply here.
struct DropArgs {
  uint32_t seed_lo, seed_hi, thr;
  float inv_keep;
};
static DropArgs drop_args(double p, int64_t seed) {
  TORCH_CHECK(p > 0.0 && p < 1.0, "attn dropout: 0 < p < 1 required (got ", p, ")");
  const uint64_t s = (uint64_t)seed;
  return {(uint32_t)s, (uint32_t)(s >> 32), attn_drop_threshold(p),
          (float)(1.0 / (1.0 - p))};
}

static void attn_fwd_dropout_launch(torch::Tensor q, torch::Tensor k, const u16* vp,
                                    AttnStrides sv, u16* op, AttnStrides so,
                                    torch::Tensor lse, const DropArgs& d) {
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  const int NW = (T % 256 == 0) ? 8 : 4;
  long grid = (long)B * H * (T / (NW * 32));
  size_t smem = std::max((size_t)(4 * 32 * C * 2), (size_t)(NW * 32 * 32 * 4));
#define LAUNCH_FWD_DROP(CC, NN)                                                 \
  hipLaunchKernelGGL((attn_fwd_kernel<CC, NN, 1, 2, true>), dim3(grid),         \
                     dim3(NN * 64), smem, cur_stream(),                         \
                     (const u16*)q.data_ptr(), (const u16*)k.data_ptr(),        \
                     vp, op,              \
                     lse.data_ptr<float>(), B, H, T, sv, so, d.seed_lo, d.seed_hi,      \
                     d.thr, d.inv_keep)
  if (C == 128 && NW == 8) LAUNCH_FWD_DROP(128, 8);
  else if (C == 128) LAUNCH_FWD_DROP(128, 4);
  else if (NW == 8) LAUNCH_FWD_DROP(64, 8);
  else LAUNCH_FWD_DROP(64, 4);
#undef LAUNCH_FWD_DROP
  launch_check();
  return;
}

std::vector<torch::Tensor> attn_fwd_dropout(torch::Tensor q, torch::Tensor k,
                                            torch::Tensor v, double p, int64_t seed) {
  CHECK_GPU(q); CHECK_GPU(k); CHECK_GPU(v);
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "attn: bf16 required");
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  TORCH_CHECK(T % 128 == 0, "attn: T % 128 == 0 required (got ", T, ")");
  TORCH_CHECK(C == 64 || C == 128, "attn: head dim 64 or 128 (got ", C, ")");
  const DropArgs d = drop_args(p, seed);
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, H, T}, q.options().dtype(torch::kFloat));
  const AttnStrides st = strides_bhtc(H, T, C);
  attn_fwd_dropout_launch(q, k, (const u16*)v.data_ptr(), st, (u16*)o.data_ptr(), st,
                          lse, d);
  return {o, lse};
}

static std::vector<torch::Tensor> attn_bwd_dropout_launch(
    const u16* dop, AttnStrides sdo, torch::Tensor q, torch::Tensor k,
    const u16* vp, AttnStrides sv, const u16* op, AttnStrides so,
    torch::Tensor lse, u16* dvp, AttnStrides sdv, const DropArgs& d,
    u16* do_copy = nullptr) {
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  long N = (long)B * H * T;
  auto delta = torch::empty({B, H, T}, q.options().dtype(torch::kFloat));
  TORCH_CHECK(N < (1L << 31), "attn: B*H*T must be below 2^31");
  long dgrid = std::min((N + 3) / 4, (long)8192);
  hipLaunchKernelGGL(attn_delta_kernel, dim3(dgrid), dim3(256), 0, cur_stream(),
                     dop, op,
                     delta.data_ptr<float>(), N, C, H, T, sdo, so, do_copy,
                     (int)(sdo.h < sdo.r));
  launch_check();
  if (do_copy) {  // the delta kernel left dO as packed (B,H,T,C) there
    dop = do_copy;
    sdo = strides_bhtc(H, T, C);
  }
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  const int NW = (T % 256 == 0) ? 8 : 4;
  long grid = (long)B * H * (T / (NW * 32));
  size_t smem_a = std::max((size_t)(2 * 4 * 32 * C) * 2 + 2 * 64 * 4,
                           (size_t)(NW * 32 * 32 * 4));
  size_t smem_b = std::max((size_t)(2 * 3 * 32 * C) * 2 + NW * 32 * 32 * 2,
                           (size_t)(NW * 32 * 32 * 4));
#define LAUNCH_BWD_DROP(CC, NN)                                                 \
  do {                                                                          \
    if (smem_a > 64 * 1024)                                                     \
      hipFuncSetAttribute(reinterpret_cast<const void*>(                        \
                              &attn_bwd_dkv_kernel<CC, NN, 0, 2, true>),        \
                          hipFuncAttributeMaxDynamicSharedMemorySize,           \
                          (int)smem_a);                                         \
    if (smem_b > 64 * 1024)                                                     \
      hipFuncSetAttribute(reinterpret_cast<const void*>(                        \
                              &attn_bwd_dq_kernel<CC, NN, 1, 2, true>),         \
                          hipFuncAttributeMaxDynamicSharedMemorySize,           \
                          (int)smem_b);                                         \
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<CC, NN, 0, 2, true>), dim3(grid),   \
                       dim3(NN * 64), smem_a, cur_stream(),                     \
                       dop, (const u16*)q.data_ptr(),     \
                       (const u16*)k.data_ptr(), vp,      \
                       lse.data_ptr<float>(), delta.data_ptr<float>(),          \
                       (u16*)dk.data_ptr(), dvp, B, H, T,       \
                       sdo, sv, sdv, d.seed_lo, d.seed_hi, d.thr, d.inv_keep);                \
    hipLaunchKernelGGL((attn_bwd_dq_kernel<CC, NN, 1, 2, true>), dim3(grid),    \
                       dim3(NN * 64), smem_b, cur_stream(),                     \
                       dop, (const u16*)q.data_ptr(),     \
                       (const u16*)k.data_ptr(), vp,      \
                       lse.data_ptr<float>(), delta.data_ptr<float>(),          \
                       (u16*)dq.data_ptr(), B, H, T, sdo, sv, d.seed_lo, d.seed_hi,      \
                       d.thr, d.inv_keep);                                      \
  } while (0)
  if (C == 128 && NW == 8) LAUNCH_BWD_DROP(128, 8);
  else if (C == 128) LAUNCH_BWD_DROP(128, 4);
  else if (NW == 8) LAUNCH_BWD_DROP(64, 8);
  else LAUNCH_BWD_DROP(64, 4);
#undef LAUNCH_BWD_DROP
  launch_check();
  return {dq, dk};
}

std::vector<torch::Tensor> attn_bwd_dropout(torch::Tensor dO, torch::Tensor q,
                                            torch::Tensor k, torch::Tensor v,
                                            torch::Tensor o, torch::Tensor lse,
                                            double p, int64_t seed) {
  CHECK_GPU(dO); CHECK_GPU(q); CHECK_GPU(k); CHECK_GPU(v); CHECK_GPU(o); CHECK_GPU(lse);
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "attn: bf16 required");
  int H = q.size(1), T = q.size(2), C = q.size(3);
  TORCH_CHECK(T % 128 == 0, "attn: T % 128 == 0 required (got ", T, ")");
  TORCH_CHECK(C == 64 || C == 128, "attn: head dim 64 or 128 (got ", C, ")");
  const DropArgs d = drop_args(p, seed);
  auto dv = torch::empty_like(v);
  const AttnStrides st = strides_bhtc(H, T, C);
  auto r = attn_bwd_dropout_launch((const u16*)dO.data_ptr(), st, q, k,
                                   (const u16*)v.data_ptr(), st,
                                   (const u16*)o.data_ptr(), st, lse,
                                   (u16*)dv.data_ptr(), st, d);
  return {r[0], r[1], dv};
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
  CHECK_GPU(v);
  TORCH_CHECK(v.scalar_type() == torch::kBFloat16 && v.sizes() == q.sizes(),
              "attn: v must be bf16 (B,H,T,C) like q, or the packed (B,T,3,H,C) qkv");
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
  const AttnStrides so = strides_bthc(H, T, C);
  if (p > 0.0)
    attn_fwd_dropout_launch(q, k, vp, sv, (u16*)o.data_ptr(), so, lse, drop_args(p, seed));
  else
    attn_fwd_launch(q, k, vp, sv, (u16*)o.data_ptr(), so, lse);
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
  CHECK_GPU(lse);
  int B = q.size(0), H = q.size(1), T = q.size(2), C = q.size(3);
  TORCH_CHECK(lse.scalar_type() == torch::kFloat && lse.numel() == (long)B * H * T,
              "attn: lse must be fp32 (B,H,T)");
  u16* dvp = (u16*)dqkv.data_ptr() + 2L * H * C;
  const AttnStrides sdv = strides_qkv_slot(H, T, C), so = strides_bthc(H, T, C);
  torch::Tensor do_copy;
  u16* dcp = nullptr;
  if (stage_do) {
    do_copy = torch::empty_like(q);
    dcp = (u16*)do_copy.data_ptr();
  }
  if (p > 0.0)
    return attn_bwd_dropout_launch((const u16*)dO.data_ptr(), so, q, k, vp, sv,
                                   (const u16*)o.data_ptr(), so, lse, dvp, sdv,
                                   drop_args(p, seed), dcp);
  return attn_bwd_launch((const u16*)dO.data_ptr(), so, q, k, vp, sv,
                         (const u16*)o.data_ptr(), so, lse, dvp, sdv, dcp);
}

// ---------------------------------------------------------------------------
torch::Tensor embedding_bwd(torch::Tensor dy, torch::Tensor idx, long V) {
  CHECK_GPU(dy); CHECK_GPU(idx);
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16, "embedding_bwd: dy bf16");
  TORCH_CHECK(idx.scalar_type() == torch::kLong, "embedding_bwd: idx int64");
  long N = dy.size(0);
  int D = dy.size(1);
  TORCH_CHECK(D % 8 == 0, "embedding_bwd: D % 8 == 0");
  static const bool use_atomic = getenv("MIDGPT_EMBED_ATOMIC") != nullptr;
  if (!use_atomic && D % 64 == 0) {
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
  static const int gnt = getenv("MIDGPT_GELU_NT") ? 1 : 0;
  if (gnt)
    hipLaunchKernelGGL((gelu_fwd_bf16<1>), dim3(grid), dim3(256), 0, cur_stream(),
                     (const u16*)x.data_ptr(), (u16*)y.data_ptr(), n);
  else
    hipLaunchKernelGGL((gelu_fwd_bf16<0>), dim3(grid), dim3(256), 0,
                       cur_stream(), (const u16*)x.data_ptr(),
                       (u16*)y.data_ptr(), n);
  launch_check();
  return y;
}

torch::Tensor gelu_bwd(torch::Tensor dy, torch::Tensor x) {
  CHECK_GPU(dy); CHECK_GPU(x);
  auto dx = torch::empty_like(x);
  long n = x.numel();
  long grid = std::min((n / 8 + 255) / 256 + 1, (long)8192);
  static const int gnt2 = getenv("MIDGPT_GELU_NT") ? 1 : 0;
  if (gnt2)
    hipLaunchKernelGGL((gelu_bwd_bf16<1>), dim3(grid), dim3(256), 0, cur_stream(),
                     (const u16*)dy.data_ptr(), (const u16*)x.data_ptr(),
                     (u16*)dx.data_ptr(), n);
  else
    hipLaunchKernelGGL((gelu_bwd_bf16<0>), dim3(grid), dim3(256), 0,
                       cur_stream(), (const u16*)dy.data_ptr(),
                       (const u16*)x.data_ptr(), (u16*)dx.data_ptr(), n);
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

// sin/cos are the FULL tables (rows >= pos+Tn, C/2) fp32; fp32 LN weights are
// used in place, others converted.
torch::Tensor kv_append(torch::Tensor qkv, torch::Tensor qw, torch::Tensor kw,
                        torch::Tensor sin_t, torch::Tensor cos_t,
                        torch::Tensor k_cache, torch::Tensor v_cache, int64_t pos,
                        double eps) {
  CHECK_GPU(qkv); CHECK_GPU(sin_t); CHECK_GPU(cos_t); CHECK_GPU(qw); CHECK_GPU(kw);
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16, "kv_append: qkv must be bf16");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "kv_append: qkv must be (B,Tn,3,H,C)");
  int B = qkv.size(0), Tn = qkv.size(1), H = qkv.size(3), C = qkv.size(4);
  check_decode_cache(k_cache, v_cache, B, H, C, "kv_append");
  const int64_t Tmax = k_cache.size(2);
  TORCH_CHECK(Tn >= 1, "kv_append: no new tokens");
  TORCH_CHECK(pos >= 0 && pos + Tn <= Tmax, "kv_append: rows [", pos, ", ", pos + Tn,
              ") do not fit a cache of ", Tmax, " rows");
  TORCH_CHECK(qw.numel() == C && kw.numel() == C, "kv_append: LN weights must be (C,)");
  TORCH_CHECK(sin_t.scalar_type() == torch::kFloat && cos_t.scalar_type() == torch::kFloat &&
              sin_t.dim() == 2 && sin_t.size(1) == C / 2 && cos_t.sizes() == sin_t.sizes(),
              "kv_append: sin/cos must be fp32 (rows, C/2)");
  TORCH_CHECK(sin_t.size(0) >= pos + Tn, "kv_append: sin/cos tables have ", sin_t.size(0),
              " rows, position ", pos + Tn - 1, " needed");
  auto q = torch::empty({B, H, Tn, C}, qkv.options());
  auto qwf = qw.to(torch::kFloat);
  auto kwf = kw.to(torch::kFloat);
  const long nrows = (long)B * Tn * H * 3;
  const int rpb = 4 * (WAVE / (C / 8));  // rows per 256-thread block
  const long grid = std::min((nrows + rpb - 1) / rpb, (long)16384);
  hipLaunchKernelGGL(kv_append_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                     (const u16*)qkv.data_ptr(), qwf.data_ptr<float>(),
                     kwf.data_ptr<float>(), sin_t.data_ptr<float>(),
                     cos_t.data_ptr<float>(), (u16*)q.data_ptr(),
                     (u16*)k_cache.data_ptr(), (u16*)v_cache.data_ptr(),
                     B, Tn, H, C, (long)Tmax, (long)pos, (float)eps);
  launch_check();
  return q;
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
// [0, kv_len - Tq + i]. Returns o (B,Tq,H,C).
torch::Tensor attn_decode(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                          int64_t kv_len, int64_t num_splits) {
  CHECK_GPU(q);
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "attn_decode: q must be bf16");
  TORCH_CHECK(q.dim() == 4, "attn_decode: q must be (B,H,Tq,C)");
  int B = q.size(0), H = q.size(1), Tq = q.size(2), C = q.size(3);
  check_decode_cache(k_cache, v_cache, B, H, C, "attn_decode");
  const int64_t Tmax = k_cache.size(2);
  TORCH_CHECK(kv_len <= Tmax, "attn_decode: kv_len ", kv_len, " exceeds the cache (", Tmax, ")");
  TORCH_CHECK(Tq >= 1 && Tq <= 16 && Tq <= kv_len,
              "attn_decode: 1 <= Tq <= min(16, kv_len) required (Tq ", Tq, ", kv_len ",
              kv_len, ")");
  TORCH_CHECK(num_splits >= 0 && num_splits <= DECODE_MAX_SPLITS,
              "attn_decode: num_splits must be in [0, ", DECODE_MAX_SPLITS, "]");
  const long rows = (long)B * H * Tq;
  TORCH_CHECK(rows > 0 && rows < (1L << 31) && kv_len < (1L << 31),
              "attn_decode: size out of range");
  if (num_splits == 0)
    num_splits = attn_decode_auto_splits(rows, kv_len, decode_cu_count());
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
#define LAUNCH_DECODE(CC)                                                         \
  hipLaunchKernelGGL(attn_decode_kernel<CC>, dim3(rows, S), dim3(256), 0,         \
                     cur_stream(), (const u16*)q.data_ptr(),                      \
                     (const u16*)k_cache.data_ptr(), (const u16*)v_cache.data_ptr(), \
                     (u16*)o.data_ptr(), accp, mlp, H, Tq, (long)Tmax, (int)kv_len, \
                     S, scale)
  if (C == 128) LAUNCH_DECODE(128);
  else LAUNCH_DECODE(64);
#undef LAUNCH_DECODE
  launch_check();
  if (S > 1) {
    hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(rows), dim3(C), 0, cur_stream(),
                       accp, mlp, (u16*)o.data_ptr(), H, Tq, C, S);
    launch_check();
  }
  return o;
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
  mod.def("attn_decode_auto_splits", &attn_decode_auto_splits, py::arg("rows"),
          py::arg("kv_len"), py::arg("cus"));
  mod.def("embedding_bwd", &embedding_bwd);
  mod.def("gelu_fwd", &gelu_fwd);
  mod.def("gelu_bwd", &gelu_bwd);
  mod.def("linear_gelu_fwd", &linear_gelu_fwd);
  mod.def("lt_probe", &lt_probe);
  mod.def("matmul_dgelu", &matmul_dgelu);
  mod.def("probe_mfma", &probe_mfma);
  mod.def("probe_pack", &probe_pack);
}
