// Python bindings for the runbooks_amd CDNA4 (gfx950) kernel library.

#include <torch/extension.h>

std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor w, double eps);
std::vector<at::Tensor> rmsnorm_fwd_dec(at::Tensor x, at::Tensor w, double eps);
std::vector<at::Tensor> rmsnorm_res_fwd_dec(at::Tensor x, at::Tensor res, at::Tensor w, double eps);
std::vector<at::Tensor> rmsnorm_res_slab_fwd_dec(at::Tensor x, at::Tensor slabs, at::Tensor w, double eps);
at::Tensor decode_gemm_raw(at::Tensor xs, at::Tensor ws, int64_t M, int64_t N, int64_t K,
                           int64_t layout, int64_t hq, int64_t hkv, int64_t dh);
at::Tensor decode_gemm_glu(at::Tensor xs, at::Tensor ws, int64_t M, int64_t N, int64_t K,
                           bool gelu);
at::Tensor decode_gemm_rope_append(at::Tensor xs, at::Tensor ws, int64_t M, int64_t N,
                                   int64_t K, at::Tensor cos, at::Tensor sin,
                                   at::Tensor positions, at::Tensor k_cache,
                                   at::Tensor v_cache, at::Tensor slot_mapping,
                                   int64_t hq);
at::Tensor decode_swizzle_w_layout(at::Tensor w, int64_t layout, int64_t hq, int64_t hkv,
                                   int64_t dh);
at::Tensor lora_delta_(at::Tensor y, at::Tensor t, at::Tensor w, double scale, bool w_transposed);
at::Tensor lora_badd_(at::Tensor y, at::Tensor t, at::Tensor w, double scale);
at::Tensor lora_shrink(at::Tensor x, at::Tensor a_stack, at::Tensor idx, int64_t S);
at::Tensor lora_expand_(at::Tensor y, at::Tensor t, at::Tensor b_stack, at::Tensor scales,
                        at::Tensor idx, std::vector<int64_t> seg_ends);
std::vector<at::Tensor> swiglu_packed_dec(at::Tensor y);
std::vector<at::Tensor> geglu_packed_dec(at::Tensor y);
std::vector<at::Tensor> rmsnorm_bwd(at::Tensor x, at::Tensor w, at::Tensor dy,
                                    at::Tensor inv_rms);
at::Tensor rope_fwd(at::Tensor x, at::Tensor cos, at::Tensor sin,
                    at::Tensor positions, int64_t heads);
at::Tensor rope_bwd(at::Tensor dy, at::Tensor cos, at::Tensor sin,
                    at::Tensor positions, int64_t heads);
void adamw_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                double lr, double beta1, double beta2, double eps, double wd,
                int64_t step);
void adamw_step_multi(at::Tensor table, int64_t nchunks, bool p32, bool g32,
                      double lr, double beta1, double beta2, double eps,
                      double wd, int64_t step);
int64_t adamw_mt_chunk_elems();
at::Tensor sample_tokens(at::Tensor logits, double temperature, int64_t seed);
at::Tensor sample_batch(at::Tensor logits, at::Tensor params_cpu,
                        c10::optional<at::Tensor> pen_cpu, int64_t num_logprobs);
void kv_append(at::Tensor k, at::Tensor v, at::Tensor k_cache, at::Tensor v_cache,
               at::Tensor slot_mapping);
at::Tensor paged_decode(at::Tensor q, at::Tensor k_cache, at::Tensor v_cache,
                        at::Tensor block_tables, at::Tensor seq_lens,
                        int64_t nsplit, double scale,
                        c10::optional<at::Tensor> seq_starts);
std::vector<at::Tensor> paged_decode_swz(at::Tensor q, at::Tensor k_cache,
                                         at::Tensor v_cache,
                                         at::Tensor block_tables,
                                         at::Tensor seq_lens, int64_t nsplit,
                                         double scale,
                                         c10::optional<at::Tensor> seq_starts);
at::Tensor paged_verify(at::Tensor q, at::Tensor k_cache, at::Tensor v_cache,
                        at::Tensor block_tables, at::Tensor seq_lens,
                        at::Tensor q_lens, int64_t nsplit, double scale);
at::Tensor flash_prefill(at::Tensor q, at::Tensor k, at::Tensor v, double scale);
at::Tensor flash_prefill_paged(at::Tensor q, at::Tensor k_cache, at::Tensor v_cache,
                               at::Tensor block_table, int64_t ctx_len, double scale);
at::Tensor flash_prefill_paged_batch(at::Tensor q, at::Tensor k_cache,
                                     at::Tensor v_cache, at::Tensor block_tables,
                                     at::Tensor plan_dev, at::Tensor plan_cpu,
                                     int64_t B, double scale);
std::vector<at::Tensor> flash_fwd_train(at::Tensor q, at::Tensor k, at::Tensor v,
                                        double scale);
std::vector<at::Tensor> fa_bwd(at::Tensor dout, at::Tensor q, at::Tensor k,
                               at::Tensor v, at::Tensor out, at::Tensor lse,
                               double scale);
at::Tensor swiglu_fwd(at::Tensor g, at::Tensor u);
std::vector<at::Tensor> swiglu_bwd(at::Tensor dy, at::Tensor g, at::Tensor u);
std::vector<at::Tensor> cross_entropy_fwd(at::Tensor logits, at::Tensor targets,
                                          int64_t ignore_index);
at::Tensor cross_entropy_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                             double gscale, int64_t ignore_index);
at::Tensor mfma_probe_32x32x16(at::Tensor a, at::Tensor b);
at::Tensor mfma_probe_16x16x32(at::Tensor a, at::Tensor b);
at::Tensor train_gemm_nt(at::Tensor a, at::Tensor b);
at::Tensor skinny_gemm(at::Tensor x, at::Tensor w);
at::Tensor decode_gemm(at::Tensor xs, at::Tensor ws, int64_t M, int64_t N, int64_t K, int64_t force_split,
                       int64_t layout, int64_t hq, int64_t hkv, int64_t dh, int64_t u,
                       int64_t tail);
at::Tensor decode_swizzle_w(at::Tensor w);
at::Tensor decode_swizzle_x(at::Tensor x);
int64_t decode_gemm_split(int64_t N, int64_t K);
bool decode_gemm_supported(int64_t M, int64_t N, int64_t K);
at::Tensor skinny_gemm_fp8(at::Tensor x, at::Tensor w8, at::Tensor scale);
std::vector<at::Tensor> w4_swizzle(at::Tensor q, at::Tensor scales);
at::Tensor decode_gemm_w4(at::Tensor xs, at::Tensor wq_swz, at::Tensor sc_swz,
                          int64_t M, int64_t N, int64_t K, int64_t force_split,
                          int64_t tail);
int64_t decode_gemm_w4_split(int64_t N, int64_t K);
bool decode_gemm_w4_supported(int64_t M, int64_t N, int64_t K);
at::Tensor gemm_w4(at::Tensor x, at::Tensor wq_swz, at::Tensor sc_swz,
                   int64_t N, int64_t K);
bool gemm_w4_supported(int64_t M, int64_t N, int64_t K);
int64_t skinny_gemm_mmax();
at::Tensor qkv_rope_append(at::Tensor y, at::Tensor cos, at::Tensor sin,
                           at::Tensor positions, at::Tensor k_cache,
                           at::Tensor v_cache, at::Tensor slot_mapping,
                           int64_t hq);
at::Tensor swiglu_packed(at::Tensor y);
at::Tensor geglu_packed(at::Tensor y);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "runbooks_amd gfx950 HIP kernels";
  m.def("rmsnorm_fwd", &rmsnorm_fwd, "fused RMSNorm forward (bf16/f32)");
  m.def("rmsnorm_fwd_dec", &rmsnorm_fwd_dec,
        "RMSNorm forward + decode-GEMM operand swizzle in one pass");
  m.def("rmsnorm_res_fwd_dec", &rmsnorm_res_fwd_dec,
        "residual add + RMSNorm + decode operand swizzle in one pass");
  m.def("rmsnorm_res_slab_fwd_dec", &rmsnorm_res_slab_fwd_dec,
        "split-K slab combine + residual + RMSNorm + swizzle in one pass");
  m.def("decode_gemm_raw", &decode_gemm_raw,
        "decode GEMM returning the uncombined fp32 slab at split>1",
        py::arg("xs"), py::arg("ws"), py::arg("M"), py::arg("N"),
        py::arg("K"), py::arg("layout") = 0, py::arg("hq") = 0,
        py::arg("hkv") = 0, py::arg("dh") = 0);
  m.def("decode_gemm_glu", &decode_gemm_glu,
        "gate-up decode GEMM (glu16 weight) + fused SwiGLU/GeGLU epilogue "
        "-> down-proj decode operand",
        py::arg("xs"), py::arg("ws"), py::arg("M"), py::arg("N"),
        py::arg("K"), py::arg("gelu") = false);
  m.def("decode_gemm_rope_append", &decode_gemm_rope_append,
        "qkv decode GEMM (rope16 weight) + fused RoPE and paged KV append "
        "-> rope'd q");
  m.def("decode_swizzle_w_layout", &decode_swizzle_w_layout,
        "one-time [N,K] -> row-permuted fragment-lane-major weight layout "
        "(0 plain, 1 glu16, 2 rope16)",
        py::arg("w"), py::arg("layout"), py::arg("hq") = 0,
        py::arg("hkv") = 0, py::arg("dh") = 0);
  m.def("lora_delta_", &lora_delta_,
        "in-place y += scale * t[T,r<=32] @ W[N,r]^T (LoRA merge)");
  m.def("lora_badd_", &lora_badd_,
        "MFMA in-place y += scale * t[T,16] @ W[N,16]^T (LoRA B merge)");
  m.def("lora_shrink", &lora_shrink,
        "per-row LoRA A product: t[M,S*R] = x[M,K] @ a_stack[idx[m]]^T (fp32 out)",
        py::arg("x"), py::arg("a_stack"), py::arg("idx"), py::arg("S"));
  m.def("lora_expand_", &lora_expand_,
        "per-row LoRA B merge, in place: y[m] += scales[idx[m]] * t[m] @ "
        "b_stack[idx[m]]^T per segment",
        py::arg("y"), py::arg("t"), py::arg("b_stack"), py::arg("scales"),
        py::arg("idx"), py::arg("seg_ends"));
  m.def("swiglu_packed_dec", &swiglu_packed_dec,
        "packed SwiGLU + decode-GEMM operand swizzle in one pass");
  m.def("geglu_packed_dec", &geglu_packed_dec,
        "packed GeGLU + decode-GEMM operand swizzle in one pass");
  m.def("rmsnorm_bwd", &rmsnorm_bwd, "fused RMSNorm backward");
  m.def("rope_fwd", &rope_fwd, "RoPE rotate-half forward");
  m.def("rope_bwd", &rope_bwd, "RoPE rotate-half backward (inverse rotation)");
  m.def("adamw_step", &adamw_step, "fused AdamW single-tensor step");
  m.def("adamw_step_multi", &adamw_step_multi,
        "fused AdamW multi-tensor step over a cached chunk table");
  m.def("adamw_mt_chunk_elems", &adamw_mt_chunk_elems,
        "elements per multi-tensor chunk");
  m.def("sample_tokens", &sample_tokens, "greedy / Gumbel-max sampling");
  m.def("sample_batch", &sample_batch,
        "batched per-row sampler: penalties, top-k/top-p/min-p, draw, "
        "logprobs -> packed int32 [B, 4 + 2L]",
        py::arg("logits"), py::arg("params_cpu"),
        py::arg("pen_cpu") = py::none(), py::arg("num_logprobs") = 0);
  m.def("kv_append", &kv_append, "paged KV-cache append");
  m.def("paged_decode", &paged_decode, "paged GQA/MQA decode attention",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_tables"), py::arg("seq_lens"), py::arg("nsplit"),
        py::arg("scale"), py::arg("seq_starts") = py::none());
  m.def("paged_decode_swz", &paged_decode_swz,
        "paged decode also emitting the o_proj decode-GEMM operand",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_tables"), py::arg("seq_lens"), py::arg("nsplit"),
        py::arg("scale"), py::arg("seq_starts") = py::none());
  m.def("paged_verify", &paged_verify,
        "multi-query paged decode attention (speculative verify): up to 8 "
        "query rows per sequence, all lengths on the device",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_tables"), py::arg("seq_lens"), py::arg("q_lens"),
        py::arg("nsplit"), py::arg("scale"));
  m.def("flash_prefill", &flash_prefill, "MFMA flash-attention prefill (causal)");
  m.def("flash_prefill_paged", &flash_prefill_paged,
        "MFMA flash-attention prefill of one chunk over the paged KV cache",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_table"), py::arg("ctx_len"), py::arg("scale"));
  m.def("flash_prefill_paged_batch", &flash_prefill_paged_batch,
        "MFMA flash-attention prefill of several sequences' packed chunks "
        "over the paged KV cache",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_tables"), py::arg("plan_dev"), py::arg("plan_cpu"),
        py::arg("num_seqs"), py::arg("scale"));
  m.def("flash_fwd_train", &flash_fwd_train,
        "MFMA flash-attention forward + log-sum-exp (training)");
  m.def("fa_bwd", &fa_bwd,
        "MFMA flash-attention backward -> (dq, dk_perq, dv_perq)");
  m.def("swiglu_fwd", &swiglu_fwd, "fused silu(g)*u");
  m.def("swiglu_bwd", &swiglu_bwd, "fused SwiGLU backward");
  m.def("cross_entropy_fwd", &cross_entropy_fwd, "fused CE: per-row loss + lse");
  m.def("cross_entropy_bwd", &cross_entropy_bwd, "fused CE backward -> dlogits");
  m.def("mfma_probe_16x16x32", &mfma_probe_16x16x32,
        "layout probe: one 16x16x32 bf16 MFMA as a plain matmul");
  m.def("mfma_probe_32x32x16", &mfma_probe_32x32x16,
        "layout probe: one 32x32x16 bf16 MFMA as a plain matmul");
  m.def("skinny_gemm", &skinny_gemm,
        "HBM-rate decode GEMM: y[M<=32,N] = x @ W^T (bf16)");
  m.def("skinny_gemm_mmax", &skinny_gemm_mmax);
  m.def("decode_gemm", &decode_gemm,
        "v2 weight-stream decode GEMM over pre-swizzled operands: "
        "y[M<=32,N] = x @ W^T (bf16), 1KiB coalesced nt weight bursts",
        py::arg("xs"), py::arg("ws"), py::arg("M"), py::arg("N"),
        py::arg("K"), py::arg("force_split") = -1, py::arg("layout") = 0,
        py::arg("hq") = 0, py::arg("hkv") = 0, py::arg("dh") = 0,
        py::arg("u") = 0, py::arg("tail") = -1);
  m.def("decode_swizzle_w", &decode_swizzle_w,
        "one-time [N,K] -> fragment-lane-major weight layout");
  m.def("decode_swizzle_x", &decode_swizzle_x,
        "per-call x -> B-fragment lane order (zero-padded to M=32)");
  m.def("decode_gemm_split", &decode_gemm_split);
  m.def("decode_gemm_supported", &decode_gemm_supported);
  m.def("mfma_probe_16x16x32", &mfma_probe_16x16x32,
        "layout probe: one 16x16x32 bf16 MFMA as a plain matmul");
  m.def("train_gemm_nt", &train_gemm_nt,
        "EXPERIMENTAL 256^2 8-phase bf16 GEMM (C = A @ B^T)");
  m.def("skinny_gemm_fp8", &skinny_gemm_fp8,
        "fp8-e4m3 weight-only decode GEMM with per-channel scales");
  m.def("w4_swizzle", &w4_swizzle,
        "one-time canonical int4 (q, scales) -> fragment-lane-major layout");
  m.def("decode_gemm_w4", &decode_gemm_w4,
        "int4 weight-only decode GEMM (group-64 bf16 scales): "
        "y[M<=32,N] = x @ dequant(Wq)^T (bf16)",
        py::arg("xs"), py::arg("wq_swz"), py::arg("sc_swz"), py::arg("M"),
        py::arg("N"), py::arg("K"), py::arg("force_split") = -1,
        py::arg("tail") = -1);
  m.def("decode_gemm_w4_split", &decode_gemm_w4_split);
  m.def("decode_gemm_w4_supported", &decode_gemm_w4_supported);
  m.def("gemm_w4", &gemm_w4,
        "int4 weight-only MFMA GEMM, any M, over the decode kernel's stored "
        "copy: y[M,N] = x[M,K] @ dequant(Wq)^T (bf16)",
        py::arg("x"), py::arg("wq_swz"), py::arg("sc_swz"), py::arg("N"),
        py::arg("K"));
  m.def("gemm_w4_supported", &gemm_w4_supported);
  m.def("qkv_rope_append", &qkv_rope_append,
        "packed qkv -> rope'd q + rope'd k / v appended to the paged cache");
  m.def("swiglu_packed", &swiglu_packed,
        "silu(y[:, :I]) * y[:, I:] from the fused gate/up GEMM output");
  m.def("geglu_packed", &geglu_packed,
        "packed GeGLU (tanh) epilogue [T,2I]->[T,I]");
}
