// hipBLASLt epilogue-fused GEMM for the MLP backward (plan K7: the GELU
// backward lives in the GEMM epilogue, not a separate elementwise pass).
//   matmul_dgelu    : dh = dgelu(dy @ w2, aux=h)   (the dgrad GEMM of the
//                     second linear fused with the GELU backward)
// The forward counterpart (GELU_AUX) has no gfx950 algorithm on ROCm 7.2;
// lt_probe below is how that was found.
// Row-major torch tensors are fed to hipBLASLt as their column-major
// transposes (C_rm(M,N) == C_cm(N,M)).
#include <hipblaslt/hipblaslt.h>

#include <map>
#include <mutex>
#include <tuple>

namespace blaslt {

static hipblasLtHandle_t handle() {
  static hipblasLtHandle_t h = [] {
    hipblasLtHandle_t hh;
    TORCH_CHECK(hipblasLtCreate(&hh) == HIPBLAS_STATUS_SUCCESS,
                "hipblasLtCreate failed");
    return hh;
  }();
  return h;
}

struct AlgoKey {
  long m, n, k;
  int epi;
  bool operator<(const AlgoKey& o) const {
    return std::tie(m, n, k, epi) < std::tie(o.m, o.n, o.k, o.epi);
  }
};
static std::map<AlgoKey, hipblasLtMatmulAlgo_t> algo_cache;
static std::mutex algo_mu;

static constexpr size_t WORKSPACE = 64u << 20;

// C_cm(m,n) = opA(A) x opB(B) with optional epilogue + aux. All bf16,
// fp32 compute. lda/ldb are the column-major leading dims of the STORED
// arrays; opA applies on top.
static void lt_matmul(int64_t m, int64_t n, int64_t k,
                      const void* A, hipblasOperation_t opA, int64_t lda,
                      const void* B, hipblasOperation_t opB, int64_t ldb,
                      void* C, int64_t ldc,
                      hipblasLtEpilogue_t epi, void* aux, int64_t aux_ld,
                      void* workspace, hipStream_t stream) {
  hipblasLtMatmulDesc_t desc;
  TORCH_CHECK(hipblasLtMatmulDescCreate(&desc, HIPBLAS_COMPUTE_32F,
                                        HIP_R_32F) == HIPBLAS_STATUS_SUCCESS);
  hipblasLtMatmulDescSetAttribute(desc, HIPBLASLT_MATMUL_DESC_TRANSA, &opA,
                                  sizeof(opA));
  hipblasLtMatmulDescSetAttribute(desc, HIPBLASLT_MATMUL_DESC_TRANSB, &opB,
                                  sizeof(opB));
  if (epi != HIPBLASLT_EPILOGUE_DEFAULT) {
    hipblasLtMatmulDescSetAttribute(desc, HIPBLASLT_MATMUL_DESC_EPILOGUE,
                                    &epi, sizeof(epi));
    if (aux) {
      hipblasLtMatmulDescSetAttribute(
          desc, HIPBLASLT_MATMUL_DESC_EPILOGUE_AUX_POINTER, &aux, sizeof(aux));
      hipblasLtMatmulDescSetAttribute(
          desc, HIPBLASLT_MATMUL_DESC_EPILOGUE_AUX_LD, &aux_ld, sizeof(aux_ld));
    }
  }
  // layouts: stored dims (rows x cols of the column-major array)
  auto mk_layout = [](int64_t r, int64_t c, int64_t ld) {
    hipblasLtMatrixLayout_t l;
    TORCH_CHECK(hipblasLtMatrixLayoutCreate(&l, HIP_R_16BF, r, c, ld) ==
                HIPBLAS_STATUS_SUCCESS);
    return l;
  };
  hipblasLtMatrixLayout_t la =
      mk_layout(opA == HIPBLAS_OP_N ? m : k, opA == HIPBLAS_OP_N ? k : m, lda);
  hipblasLtMatrixLayout_t lb =
      mk_layout(opB == HIPBLAS_OP_N ? k : n, opB == HIPBLAS_OP_N ? n : k, ldb);
  hipblasLtMatrixLayout_t lc = mk_layout(m, n, ldc);

  hipblasLtMatmulAlgo_t algo;
  {
    std::lock_guard<std::mutex> g(algo_mu);
    AlgoKey key{m, n, k, (int)epi};
    auto it = algo_cache.find(key);
    if (it == algo_cache.end()) {
      hipblasLtMatmulPreference_t pref;
      hipblasLtMatmulPreferenceCreate(&pref);
      size_t ws = WORKSPACE;
      hipblasLtMatmulPreferenceSetAttribute(
          pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &ws, sizeof(ws));
      hipblasLtMatmulHeuristicResult_t res[4];
      int found = 0;
      auto st = hipblasLtMatmulAlgoGetHeuristic(handle(), desc, la, lb, lc, lc,
                                                pref, 4, res, &found);
      hipblasLtMatmulPreferenceDestroy(pref);
      TORCH_CHECK(st == HIPBLAS_STATUS_SUCCESS && found > 0,
                  "hipblasLt heuristic found no algo (m=", m, " n=", n,
                  " k=", k, " epi=", (int)epi, ")");
      algo = res[0].algo;
      algo_cache[key] = algo;
    } else {
      algo = it->second;
    }
  }
  float alpha = 1.f, beta = 0.f;
  auto st = hipblasLtMatmul(handle(), desc, &alpha, A, la, B, lb, &beta, C, lc,
                            C, lc, &algo, workspace, WORKSPACE, stream);
  TORCH_CHECK(st == HIPBLAS_STATUS_SUCCESS, "hipblasLtMatmul failed: ", (int)st);
  hipblasLtMatrixLayoutDestroy(la);
  hipblasLtMatrixLayoutDestroy(lb);
  hipblasLtMatrixLayoutDestroy(lc);
  hipblasLtMatmulDescDestroy(desc);
}

}  // namespace blaslt

// dh(M,N) = dgelu(dy(M,N2) @ w2(N2,N), aux = h(M,N))
torch::Tensor matmul_dgelu(torch::Tensor dy, torch::Tensor w2, torch::Tensor h) {
  Call c("matmul_dgelu", dy);
  const u16* dyp = c.bf16(dy, "dy", {ANY, ANY});
  const int64_t M = dy.size(0), N2 = dy.size(1);
  const u16* w2p = c.bf16(w2, "w2", {N2, ANY});
  const int64_t N = w2.size(1);
  u16* hp = c.bf16_out(h, "h", {M, N});  // read only; the aux pointer is void*
  auto dh = torch::empty({M, N}, dy.options());
  auto ws = torch::empty({(long)blaslt::WORKSPACE},
                         dy.options().dtype(torch::kUInt8));
  // col-major: DH_cm(N,M) = W2_cm(N,N2) x DY_cm(N2,M)
  blaslt::lt_matmul(N, M, N2, w2p, HIPBLAS_OP_N, N, dyp, HIPBLAS_OP_N, N2,
                    fresh<u16>(dh), N, HIPBLASLT_EPILOGUE_DGELU, hp, N,
                    fresh<uint8_t>(ws), cur_stream());
  return dh;
}

// Probe: how many heuristic algos exist for a shape/epilogue/trans combo.
long lt_probe(long m, long n, long k, long epi, bool ta, bool tb) {
  hipblasLtMatmulDesc_t desc;
  if (hipblasLtMatmulDescCreate(&desc, HIPBLAS_COMPUTE_32F, HIP_R_32F) !=
      HIPBLAS_STATUS_SUCCESS) return -1;
  hipblasOperation_t opA = ta ? HIPBLAS_OP_T : HIPBLAS_OP_N;
  hipblasOperation_t opB = tb ? HIPBLAS_OP_T : HIPBLAS_OP_N;
  hipblasLtMatmulDescSetAttribute(desc, HIPBLASLT_MATMUL_DESC_TRANSA, &opA, sizeof(opA));
  hipblasLtMatmulDescSetAttribute(desc, HIPBLASLT_MATMUL_DESC_TRANSB, &opB, sizeof(opB));
  hipblasLtEpilogue_t e = (hipblasLtEpilogue_t)epi;
  hipblasLtMatmulDescSetAttribute(desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &e, sizeof(e));
  static float dummy_aux[4];
  void* aux = (void*)dummy_aux;
  int64_t auxld = m;
  if (epi >= 128) {  // aux-carrying epilogues
    hipblasLtMatmulDescSetAttribute(desc, HIPBLASLT_MATMUL_DESC_EPILOGUE_AUX_POINTER, &aux, sizeof(aux));
    hipblasLtMatmulDescSetAttribute(desc, HIPBLASLT_MATMUL_DESC_EPILOGUE_AUX_LD, &auxld, sizeof(auxld));
  }
  auto mk = [](int64_t r, int64_t c) {
    hipblasLtMatrixLayout_t l;
    hipblasLtMatrixLayoutCreate(&l, HIP_R_16BF, r, c, r);
    return l;
  };
  hipblasLtMatrixLayout_t la = mk(ta ? k : m, ta ? m : k);
  hipblasLtMatrixLayout_t lb = mk(tb ? n : k, tb ? k : n);
  hipblasLtMatrixLayout_t lc = mk(m, n);
  hipblasLtMatmulPreference_t pref;
  hipblasLtMatmulPreferenceCreate(&pref);
  size_t wsz = blaslt::WORKSPACE;
  hipblasLtMatmulPreferenceSetAttribute(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &wsz, sizeof(wsz));
  hipblasLtMatmulHeuristicResult_t res[8];
  int found = 0;
  auto st = hipblasLtMatmulAlgoGetHeuristic(blaslt::handle(), desc, la, lb, lc, lc, pref, 8, res, &found);
  hipblasLtMatmulPreferenceDestroy(pref);
  hipblasLtMatrixLayoutDestroy(la); hipblasLtMatrixLayoutDestroy(lb); hipblasLtMatrixLayoutDestroy(lc);
  hipblasLtMatmulDescDestroy(desc);
  if (st != HIPBLAS_STATUS_SUCCESS) return -(long)st;
  return found;
}
