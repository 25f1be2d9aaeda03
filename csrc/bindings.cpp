// genrec_amd._C — single op library for the CDNA4 kernel layer.
#include <torch/extension.h>

namespace genrec {

std::vector<torch::Tensor> rms_norm_fwd(torch::Tensor x, torch::Tensor w,
                                        double eps, bool t5_style);
std::vector<torch::Tensor> rms_norm_bwd(torch::Tensor dy, torch::Tensor x,
                                        torch::Tensor w, torch::Tensor inv_rms,
                                        bool t5_style);
std::vector<torch::Tensor> l2norm_fwd(torch::Tensor x, double eps);
torch::Tensor l2norm_bwd(torch::Tensor dy, torch::Tensor x,
                         torch::Tensor inv_norm, double eps);

std::vector<torch::Tensor> attn_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> key_pad,
    c10::optional<torch::Tensor> add_mask,
    c10::optional<torch::Tensor> query_mask,
    double scale, bool causal, int64_t act, double dropout_p, int64_t seed,
    c10::optional<torch::Tensor> seed_dev);
std::vector<torch::Tensor> attn_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor p_saved, torch::Tensor drop_mask,
    c10::optional<torch::Tensor> query_mask,
    double scale, int64_t act, double dropout_p, int64_t seed,
    bool bias_grad, int64_t bias_dim);

std::vector<torch::Tensor> attn_fwd_mfma(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> key_pad,
    c10::optional<torch::Tensor> add_mask,
    c10::optional<torch::Tensor> query_mask,
    double scale, bool causal, int64_t act, double dropout_p, int64_t seed,
    c10::optional<torch::Tensor> seed_dev,
    c10::optional<torch::Tensor> bias_bucket);
std::vector<torch::Tensor> attn_bwd_mfma(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor p_saved, torch::Tensor drop_mask,
    c10::optional<torch::Tensor> query_mask,
    double scale, int64_t act, double dropout_p, int64_t seed,
    bool bias_grad, int64_t bias_dim,
    c10::optional<torch::Tensor> bias_bucket, int64_t n_buckets,
    c10::optional<torch::Tensor> dqkv_out,
    c10::optional<torch::Tensor> dkv_out, int64_t dk_col, int64_t dv_col);
std::string attn_mfma_path(int64_t Lq, int64_t Lk, int64_t D, int64_t act,
                           bool table_mode, bool backward);

std::vector<torch::Tensor> hstu_attn_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor pos_bucket, torch::Tensor pos_table,
    c10::optional<torch::Tensor> time_table,
    c10::optional<torch::Tensor> timestamps,
    c10::optional<torch::Tensor> key_pad);
std::vector<torch::Tensor> hstu_attn_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor s_saved, torch::Tensor pos_bucket,
    c10::optional<torch::Tensor> timestamps,
    int64_t n_pos, int64_t n_time);
torch::Tensor hstu_attn_flash_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor rel_bucket, torch::Tensor pos_table,
    c10::optional<torch::Tensor> time_table,
    c10::optional<torch::Tensor> timestamps,
    c10::optional<torch::Tensor> key_pad);
std::vector<torch::Tensor> hstu_attn_flash_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor rel_bucket, torch::Tensor pos_table,
    c10::optional<torch::Tensor> time_table,
    c10::optional<torch::Tensor> timestamps,
    c10::optional<torch::Tensor> key_pad);

std::vector<torch::Tensor> softmax_ce_fwd(torch::Tensor logits,
                                          torch::Tensor targets,
                                          int64_t ignore_index);
torch::Tensor softmax_ce_bwd(torch::Tensor dloss, torch::Tensor logits,
                             torch::Tensor targets, torch::Tensor lse,
                             torch::Tensor n_valid, int64_t ignore_index);
std::vector<torch::Tensor> lce_inplace(torch::Tensor logits,
                                       torch::Tensor targets,
                                       torch::Tensor inv_n,
                                       int64_t ignore_index, int64_t slices);
int64_t lce_pick_slices(int64_t R, int64_t V);

std::vector<torch::Tensor> sqdist_argmin(torch::Tensor x,
                                         torch::Tensor codebook);
torch::Tensor embedding_fwd(torch::Tensor weight, torch::Tensor indices);
torch::Tensor embedding_bwd(torch::Tensor dy, torch::Tensor indices,
                            int64_t num_weights, int64_t padding_idx);
std::vector<torch::Tensor> dropout_add_fwd(
    torch::Tensor x, torch::Tensor residual, double p, int64_t seed,
    c10::optional<torch::Tensor> seed_dev);
std::vector<torch::Tensor> relu_dropout_fwd(
    torch::Tensor x, double p, int64_t seed,
    c10::optional<torch::Tensor> seed_dev);
std::vector<torch::Tensor> plain_dropout_fwd(
    torch::Tensor x, double p, int64_t seed,
    c10::optional<torch::Tensor> seed_dev);
torch::Tensor colsum(torch::Tensor x);
torch::Tensor chunk_sum(torch::Tensor x);
torch::Tensor seq_sum_bf16(torch::Tensor x, bool reverse);
std::vector<torch::Tensor> layer_norm_fwd(torch::Tensor x, torch::Tensor w,
                                          torch::Tensor b, double eps);
std::vector<torch::Tensor> layer_norm_bwd(torch::Tensor dy, torch::Tensor x,
                                          torch::Tensor w, torch::Tensor mean,
                                          torch::Tensor rstd);
torch::Tensor dropout_fuse_bwd(torch::Tensor dy, torch::Tensor mask,
                               double p, bool relu);
std::vector<torch::Tensor> dropout_add_rms_norm_fwd(
    torch::Tensor y, torch::Tensor residual, torch::Tensor w, double p,
    double eps, bool t5_style, int64_t seed,
    c10::optional<torch::Tensor> seed_dev);
std::vector<torch::Tensor> dropout_add_rms_norm_bwd(
    torch::Tensor dn, c10::optional<torch::Tensor> dh, torch::Tensor h,
    torch::Tensor w, torch::Tensor inv_rms, torch::Tensor mask, double p);
torch::Tensor topk_hit_ranks(torch::Tensor actual, torch::Tensor topk);
void fused_adamw(torch::Tensor master, torch::Tensor grad, torch::Tensor m,
                 torch::Tensor v, torch::Tensor out_p, torch::Tensor lr,
                 torch::Tensor scale, torch::Tensor step, double beta1,
                 double beta2, double eps, double weight_decay);
torch::Tensor skinny_gemm(torch::Tensor x, torch::Tensor w,
                          c10::optional<torch::Tensor> bias);
torch::Tensor skinny_gemm_tn(torch::Tensor x, torch::Tensor w,
                             c10::optional<torch::Tensor> bias);
std::vector<torch::Tensor> attn_fwd_flash(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> key_pad,
    c10::optional<torch::Tensor> add_mask,
    c10::optional<torch::Tensor> query_mask,
    double scale, bool causal, double dropout_p, int64_t seed,
    c10::optional<torch::Tensor> seed_dev);
std::vector<torch::Tensor> attn_bwd_flash(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor s_saved, torch::Tensor ml,
    torch::Tensor drop_mask, c10::optional<torch::Tensor> query_mask,
    double scale, double dropout_p, bool bias_grad, int64_t bias_dim);

std::vector<torch::Tensor> gqa_attn_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    c10::optional<torch::Tensor> key_pad, double scale, bool causal);
std::vector<torch::Tensor> gqa_attn_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse,
    c10::optional<torch::Tensor> key_pad, double scale, bool causal);
std::vector<torch::Tensor> gqa_varlen_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor cu_seqlens, int64_t max_seqlen, double scale);
std::vector<torch::Tensor> gqa_varlen_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse, torch::Tensor cu_seqlens,
    int64_t max_seqlen, double scale);

torch::Tensor beam_attn_fwd(torch::Tensor q, torch::Tensor k_pre,
                            torch::Tensor v_pre,
                            c10::optional<torch::Tensor> pre_pad,
                            torch::Tensor k_suf, torch::Tensor v_suf,
                            torch::Tensor anc, int64_t t, double scale,
                            int64_t splits);
torch::Tensor beam_attn_varlen_fwd(torch::Tensor q, torch::Tensor k_pre,
                                   torch::Tensor v_pre,
                                   torch::Tensor cu_seqlens,
                                   int64_t max_prefix, torch::Tensor k_suf,
                                   torch::Tensor v_suf, torch::Tensor anc,
                                   int64_t t, double scale, int64_t splits);
int64_t beam_attn_pick_splits(int64_t B, int64_t Hkv, int64_t rows,
                              int64_t Lp);


std::vector<torch::Tensor> add_rms_norm_fwd(
    torch::Tensor x, c10::optional<torch::Tensor> residual, torch::Tensor w,
    double eps);
std::vector<torch::Tensor> add_rms_norm_bwd(
    torch::Tensor dn, c10::optional<torch::Tensor> dh, torch::Tensor h,
    torch::Tensor w, torch::Tensor inv_rms);
std::vector<torch::Tensor> rope_qk_fwd(torch::Tensor q, torch::Tensor k,
                                       torch::Tensor cos, torch::Tensor sin,
                                       bool inverse);
torch::Tensor swiglu_fwd(torch::Tensor gate, torch::Tensor up);
std::vector<torch::Tensor> swiglu_bwd(torch::Tensor dy, torch::Tensor gate,
                                      torch::Tensor up);

torch::Tensor lora_down(torch::Tensor x, torch::Tensor p_mat, double c,
                        double drop_p, int64_t seed);
torch::Tensor lora_up_add_(torch::Tensor y, torch::Tensor t, torch::Tensor q,
                           double c, double drop_p, int64_t seed);
torch::Tensor lora_grad(torch::Tensor t, torch::Tensor x, double c,
                        double drop_p, int64_t seed);
torch::Tensor lora_dropout_mask(int64_t M, int64_t Kw, double p,
                                int64_t seed);

}  // namespace genrec

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rms_norm_fwd", &genrec::rms_norm_fwd, "fused RMSNorm forward");
  m.def("rms_norm_bwd", &genrec::rms_norm_bwd, "fused RMSNorm backward");
  m.def("l2norm_fwd", &genrec::l2norm_fwd, "fused L2Norm forward");
  m.def("l2norm_bwd", &genrec::l2norm_bwd, "fused L2Norm backward");
  m.def("attn_fwd", &genrec::attn_fwd, "fused attention forward");
  m.def("attn_bwd", &genrec::attn_bwd, "fused attention backward");
  m.def("attn_fwd_mfma", &genrec::attn_fwd_mfma, "MFMA attention forward",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("bias"),
        py::arg("key_pad"), py::arg("add_mask"), py::arg("query_mask"),
        py::arg("scale"), py::arg("causal"), py::arg("act"),
        py::arg("dropout_p"), py::arg("seed"), py::arg("seed_dev"),
        py::arg("bias_bucket") = py::none());
  m.def("attn_bwd_mfma", &genrec::attn_bwd_mfma, "MFMA attention backward",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("p_saved"), py::arg("drop_mask"), py::arg("query_mask"),
        py::arg("scale"), py::arg("act"), py::arg("dropout_p"),
        py::arg("seed"), py::arg("bias_grad"), py::arg("bias_dim"),
        py::arg("bias_bucket") = py::none(),
        py::arg("n_buckets") = 0,
        py::arg("dqkv_out") = py::none(),
        py::arg("dkv_out") = py::none(), py::arg("dk_col") = 0,
        py::arg("dv_col") = 0);
  m.def("attn_mfma_path", &genrec::attn_mfma_path,
        "kernel family attn_fwd_mfma (attn_bwd_mfma: backward=True) runs "
        "for a shape: "
        "\"smallq\" or \"tile64\"",
        py::arg("Lq"), py::arg("Lk"), py::arg("D"), py::arg("act") = 0,
        py::arg("table_mode") = false, py::arg("backward") = false);
  m.def("hstu_attn_fwd", &genrec::hstu_attn_fwd, "HSTU fused attention fwd");
  m.def("hstu_attn_bwd", &genrec::hstu_attn_bwd, "HSTU fused attention bwd");
  m.def("hstu_attn_flash_fwd", &genrec::hstu_attn_flash_fwd,
        "tiled HSTU attention fwd (any L): out as a [B,H,L,D] view of "
        "[B,L,H,D] memory");
  m.def("hstu_attn_flash_bwd", &genrec::hstu_attn_flash_bwd,
        "tiled HSTU attention bwd: dq, dk, dv, dpos, dtime");
  m.def("softmax_ce_fwd", &genrec::softmax_ce_fwd, "fused CE forward");
  m.def("softmax_ce_bwd", &genrec::softmax_ce_bwd, "fused CE backward");
  m.def("lce_inplace", &genrec::lce_inplace,
        "in-place CE fwd+bwd over a logits chunk (lce_stats + lce_grad)",
        py::arg("logits"), py::arg("targets"), py::arg("inv_n"),
        py::arg("ignore_index"), py::arg("slices") = 0);
  m.def("lce_pick_slices", &genrec::lce_pick_slices,
        "column slices per row chosen for an [R, V] chunk");
  m.def("sqdist_argmin", &genrec::sqdist_argmin, "L2 dist + argmin");
  m.def("embedding_fwd", &genrec::embedding_fwd, "embedding gather");
  m.def("embedding_bwd", &genrec::embedding_bwd, "embedding scatter-add bwd");
  m.def("dropout_add_fwd", &genrec::dropout_add_fwd, "residual+dropout fwd");
  m.def("relu_dropout_fwd", &genrec::relu_dropout_fwd, "dropout(relu) fwd");
  m.def("plain_dropout_fwd", &genrec::plain_dropout_fwd,
        "graph-replay-safe plain dropout fwd");
  m.def("colsum", &genrec::colsum,
        "deterministic replay-safe column sum (bias grads)");
  m.def("seq_sum_bf16", &genrec::seq_sum_bf16,
        "row sum in the given order, every partial sum rounded to bf16",
        py::arg("x"), py::arg("reverse") = false);
  m.def("chunk_sum", &genrec::chunk_sum,
        "small-row-count column sum (split-K dW partials)");
  m.def("layer_norm_fwd", &genrec::layer_norm_fwd, "fused LayerNorm fwd");
  m.def("layer_norm_bwd", &genrec::layer_norm_bwd, "fused LayerNorm bwd");
  m.def("dropout_fuse_bwd", &genrec::dropout_fuse_bwd, "fused dropout bwd");
  m.def("dropout_add_rms_norm_fwd", &genrec::dropout_add_rms_norm_fwd,
        "fused residual+dropout -> RMSNorm fwd -> (h, n, mask, inv_rms)");
  m.def("dropout_add_rms_norm_bwd", &genrec::dropout_add_rms_norm_bwd,
        "fused RMSNorm bwd + dh add + dropout bwd -> (t, dy, dw)");
  m.def("topk_hit_ranks", &genrec::topk_hit_ranks, "first-match ranks");
  m.def("fused_adamw", &genrec::fused_adamw,
        "fused flat AdamW step (device lr/scale/step scalars)");
  m.def("skinny_gemm", &genrec::skinny_gemm,
        "tall-skinny linear fwd GEMM (bf16, fp32 accum)");
  m.def("skinny_gemm_tn", &genrec::skinny_gemm_tn,
        "tall-skinny dX GEMM: x[M,K] @ w[K,N] (transposed-B staging)");
  m.def("attn_fwd_flash", &genrec::attn_fwd_flash,
        "flash-tiled attention fwd (staged; GENREC_ATTN_FLASH=1)");
  m.def("attn_bwd_flash", &genrec::attn_bwd_flash,
        "flash-tiled attention bwd (staged; GENREC_ATTN_FLASH=1)");
  m.def("gqa_attn_fwd", &genrec::gqa_attn_fwd,
        "grouped-query flash attention fwd (D 64/128) -> (out, lse)");
  m.def("gqa_attn_bwd", &genrec::gqa_attn_bwd,
        "grouped-query flash attention bwd (deterministic) -> (dq, dk, dv)");
  m.def("gqa_varlen_fwd", &genrec::gqa_varlen_fwd,
        "packed-sequence causal GQA attention fwd: q[T,Hq,D], k/v[T,Hkv,D], "
        "cu_seqlens int32 [S+1] -> (out[T,Hq,D], lse[Hq,T])");
  m.def("gqa_varlen_bwd", &genrec::gqa_varlen_bwd,
        "packed-sequence causal GQA attention bwd (deterministic) -> "
        "(dq, dk, dv) as [T,H,D]");
  m.def("beam_attn_fwd", &genrec::beam_attn_fwd,
        "shared-prefix beam-search decode attention (D 64/128) -> out",
        py::arg("q"), py::arg("k_pre"), py::arg("v_pre"), py::arg("pre_pad"),
        py::arg("k_suf"), py::arg("v_suf"), py::arg("anc"), py::arg("t"),
        py::arg("scale"), py::arg("splits") = 0);
  m.def("beam_attn_varlen_fwd", &genrec::beam_attn_varlen_fwd,
        "beam-search decode attention over a packed prefill: k_pre/v_pre "
        "[Ttot,Hkv,D], cu_seqlens int32 [B+1] -> out",
        py::arg("q"), py::arg("k_pre"), py::arg("v_pre"),
        py::arg("cu_seqlens"), py::arg("max_prefix"), py::arg("k_suf"),
        py::arg("v_suf"), py::arg("anc"), py::arg("t"), py::arg("scale"),
        py::arg("splits") = 0);
  m.def("beam_attn_pick_splits", &genrec::beam_attn_pick_splits,
        "prefix splits chosen for (B, Hkv, W*g rows, Lp)");
  m.def("add_rms_norm_fwd", &genrec::add_rms_norm_fwd,
        "wide-row (d <= 4096) residual add + RMSNorm fwd -> (h, n, inv_rms)",
        py::arg("x"), py::arg("residual"), py::arg("w"), py::arg("eps"));
  m.def("add_rms_norm_bwd", &genrec::add_rms_norm_bwd,
        "RMSNorm bwd + dh add in one pass (deterministic dw) -> (dx, dw)",
        py::arg("dn"), py::arg("dh"), py::arg("h"), py::arg("w"),
        py::arg("inv_rms"));
  m.def("rope_qk_fwd", &genrec::rope_qk_fwd,
        "rotary embedding of q and k in one launch (inverse = gradient) -> "
        "(q_out, k_out) as [B,H,L,D] views of [B,L,H,D] memory",
        py::arg("q"), py::arg("k"), py::arg("cos"), py::arg("sin"),
        py::arg("inverse") = false);
  m.def("swiglu_fwd", &genrec::swiglu_fwd, "silu(gate) * up");
  m.def("swiglu_bwd", &genrec::swiglu_bwd,
        "silu(gate) * up backward, recomputed -> (dgate, dup)");
  m.def("lora_down", &genrec::lora_down,
        "T[M,r] = bf16(c * (mask.x)[M,Kw] @ p_mat[r,Kw]^T), r in 16/32/64",
        py::arg("x"), py::arg("p_mat"), py::arg("c") = 1.0,
        py::arg("drop_p") = 0.0, py::arg("seed") = 0);
  m.def("lora_up_add_", &genrec::lora_up_add_,
        "in place: y[M,Kw] = bf16(y + c * mask.(t[M,r] @ q[Kw,r]^T)) -> y",
        py::arg("y"), py::arg("t"), py::arg("q"), py::arg("c") = 1.0,
        py::arg("drop_p") = 0.0, py::arg("seed") = 0);
  m.def("lora_grad", &genrec::lora_grad,
        "G[r,Kw] = bf16(c * t[M,r]^T @ (mask.x)[M,Kw]) (deterministic)",
        py::arg("t"), py::arg("x"), py::arg("c") = 1.0,
        py::arg("drop_p") = 0.0, py::arg("seed") = 0);
  m.def("lora_dropout_mask", &genrec::lora_dropout_mask,
        "uint8 [M,Kw] keep mask of the lora kernels (tests only)",
        py::arg("M"), py::arg("Kw"), py::arg("p"), py::arg("seed"));
}
