// mmhip engine: owns the flat parameter layout, the workspace carve-up and the launch sequence of one
// forward / backward of the late-fusion model (reference models/mm_late.py:148-193 + the HF dual encoder it calls).
// Everything is enqueued on the caller's stream from this single C++ call path: no per-op host round trip.
#include <string>
#include <vector>
#include <cstdlib>
#include <cstdio>
#include "mmhip_common.h"
#include "mmhip_host.h"

using namespace mmhip;

namespace {

struct LayerOff {   // element offsets into a flat fp32 buffer
    size_t qkv_w, qkv_b, ao_w, ao_b, ln1_w, ln1_b, fc1_w, fc1_b, fc2_w, fc2_b, ln2_w, ln2_b, begin, end;
    size_t rel_table, lambda1, lambda2;      // BEiT layers only: relative position bias table, the two layer scales
};
struct BeitWs {     // BEiT layer: what mmhip_refresh_weights derives beside the operand copies (byte offsets into the workspace)
    size_t ao_b, fc2_b;      // fp32 [Hv]: lambda_1 * attention.output.dense.bias, lambda_2 * output.dense.bias
    size_t bias;             // fp32 [heads][P][ldb]: the layer's relative position bias, expanded
};
struct LayerW16 {   // 16-bit GEMM operand copies (byte offsets into the workspace)
    size_t qkv, ao, fc1, fc2, qkvT, aoT, fc1T, fc2T;
};
struct TextAct {    // saved activations of one text layer (byte offsets into the workspace)
    size_t qkv, ctx, pre1, a1, u, h, pre2, out, mean1, rstd1, mean2, rstd2, lse;
    size_t a1p, outp;      // parity mode with plane pairs: the LayerNorm outputs once more as pairs (the fp32 forms stay the residual inputs)
};
struct ImgAct {     // saved activations of one trainable image layer (pre-LN): the layer's input stream, LN1 output (plane pairs: the pair alone), qkv, ctx,
                    // the mid stream, LN2 output, the pre-GELU value u and the GELU output h; the layer's output is the next layer's x_in
    size_t x_in, ln1, qkv, ctx, lse, x_mid, ln2, u, h, mean1, rstd1, mean2, rstd2;
};

}  // namespace

struct mmhip_engine {
    mmhip_config cfg;
    std::vector<mmhip_param_info> params;
    size_t n_frozen = 0, n_train = 0;
    // offsets (elements) ---------------------------------------------------------------
    std::vector<LayerOff> vit, txt;
    size_t v_cls, v_pos, v_patch_w, v_patch_b, v_ln_w, v_ln_b, v_pool_w, v_pool_b;          // frozen
    size_t t_word, t_pos, t_type, t_eln_w, t_eln_b, t_pool_w, t_pool_b;                     // train
    size_t logit_scale, vproj_w, tproj_w;
    size_t fq_w, fq_b, fk_w, fk_b, fv_w, fv_b, fus_w, fus_b, cls_w, cls_b, tim_w, tim_b;
    size_t asp_w = 0, asp_b = 0;         // aspectattention.* (MMHIP_FUSION_ASPECT)
    size_t heads_begin, heads_end, emb_begin, emb_end;
    // bound buffers --------------------------------------------------------------------
    float* frozen = nullptr; float* train = nullptr; float* grad = nullptr;
    char* ws = nullptr; size_t ws_bytes = 0, ws_need = 0;
    // workspace offsets (bytes) --------------------------------------------------------
    std::vector<LayerW16> vit_w16, txt_w16;
    size_t x3_ws[3] = {0, 0, 0}, x3_bytes[3] = {0, 0, 0};      // parity mode: split-plane scratch of the caller's stream | side stream | image-tower stream
    size_t patch_w16;
    std::vector<TextAct> tact;
    size_t ids_all, mask_all, pos_ids, maskbias, x0, xhat_emb, rstd_emb, x0p = 0;
    // Parity mode (bf16x3), round 4: every tensor that feeds a matrix product is written by its producer as a PLANE PAIR (mmhip_kernels.h) and the
    // GEMMs read the planes directly (MMHIP_X3_PAIRS=0 at mmhip_create: round 3's form -- fp32 tensors, split into scratch copies per call).
    // Pairs: weights' operand copies, qkv, ctx, FC1 output h, the LayerNorm outputs (beside their fp32 forms), the image tower's LN output /
    // qkv / ctx / h / patches, and in the backward du, dqkv, d ctx and the LayerNorm-backward outputs the GEMMs read.  fp32: the residual
    // stream (pre1, pre2, x, d pre, dx), the GELU stash u, everything the heads touch.
    bool px = false;
    int bwd_np = 3;          // parity mode, plane pairs: products per k slice in the BACKWARD's matrix products (3 = as the forward; 2; 1) -- mmhip_set_backward_products
    size_t v_patches, v_pe, v_x, v_ln, v_qkv, v_ctx, v_h, v_out;                             // ViT ping-pong
    size_t g_partial, g_partial_side, g_det_rows = 0;
    size_t g_lnp[2][2];      // LN-backward partials per (layer parity, LN index): reduced on the side stream with the layer's dW
    uint8_t* word_row_state = nullptr;     // caller-owned row flags of the word table (mmhip_set_row_state)
    unsigned* bad_index = nullptr;         // caller-owned device word counting token ids that had to be clamped into the word table (mmhip_set_index_counter)
    unsigned* guard = nullptr;             // caller-owned overflow-guard words of THIS handle, {counter, void-step flag} (mmhip_set_guard); null: the
                                           // process-wide registration of mmhip_set_step_guard, if any
    void* clip_state = nullptr;            // caller-owned state block of global-norm gradient clipping (mmhip_set_grad_clip); null: not armed
    float clip_max = 0.f;                  // its threshold (> 0 while armed)
    size_t g_set[2][6];      // double-buffered backward temporaries read by the side stream: dpre2, ddrop2, du, dpre1, ddrop1, dqkv
    size_t g_dx, g_dx2, g_dpre, g_ddrop, g_dpre1, g_ddrop1, g_dqkv, g_dctx, g_du;                               // backward temporaries
    // heads (fp32) ----------------------------------------------------------------------
    size_t h_vpool, h_tpool, h_txt_e, h_img_e, h_txt_n, h_img_n, h_txt_inv, h_img_inv, h_logits;
    size_t h_q, h_qk, h_prob, h_xbar, h_z, h_feats, h_featd, h_out_cls, h_out_tim;
    size_t splitk_ws = 0, splitk_ws_vit = 0; bool has_splitk = false;      // fp32 scratch of the split-K path of the <= 128-row GEMMs: one per stream that
                                                                           // issues NT GEMMs (the caller's; the image tower's side stream) -- two towers' small
                                                                           // GEMMs may run side by side
    size_t h_d_out_cls, h_d_logits, h_d_out_tim, h_dfeats, h_dpre, h_dz, h_dxcls, h_dxbar, h_dqk, h_dq, h_dtxt_e, h_dimg_e,
        h_dtpool, h_dprepool, h_loss;
    size_t h_asp_w = 0, h_asp_e = 0, h_asp_partial = 0;      // aspect-att fusion: softmax weights and tanh outputs [B, 2] of the forward; d a / d b partials
    // state of the last forward --------------------------------------------------------
    int B = 0, T = 0, Bt = 0; bool itm = false, train_mode = false, fwd_done = false, bwd_begun = false;
    bool skip_itc = false, itc_done = false;   // mmhip_train_step without the ITC loss: the dual-encoder similarity head (text pooler, both projections,
                                               // normalisation, logits: five launches on the critical path between towers and backward) is not run
    uint64_t seed = 0;
    // global-batch ITC (mmhip_reserve_itc_global / mmhip_set_itc_global): slices behind ws_base, present only after a reservation
    size_t ws_base = 0;                        // workspace bytes of a handle that never reserved: build_workspace's total
    int itc_max_world = 0, itc_world = 1, itc_rank = 0;
    size_t h_g_txt = 0, h_g_img = 0, h_g_rowlse = 0, h_g_collse = 0, h_g_loss = 0, h_g_dtn = 0, h_g_din = 0, h_g_ws = 0;
    bool bd_itc_global = false; float bd_w_itc = 0.f;      // the last mmhip_loss took the gathered form: heads_backward runs launch_itc_global_bwd
    const float *bd_out_cls = nullptr, *bd_logits = nullptr, *bd_out_tim = nullptr, *bd_feats = nullptr;
    // internal side stream (ViT forward beside the text forward; weight gradients beside the dX chain) -------------
    hipStream_t side = nullptr;          // weight-gradient work of the backward
    int vision_ready_B = 0;              // > 0: the image tower's outputs for that many posts were imported (mmhip_vision_import)
    bool vit_is_long = false;            // the image tower is the longer forward chain of this call (set by mmhip_forward)
    hipStream_t side_vit[2] = {nullptr, nullptr};     // image tower of the forward: [0] normal, [1] high priority
    hipEvent_t ev_fork = nullptr, ev_vit = nullptr, ev_ready[2] = {nullptr, nullptr}, ev_tn[2] = {nullptr, nullptr};
    hipEvent_t ev_layer[2] = {nullptr, nullptr}, ev_opt = nullptr;      // mmhip_train_step: per-layer AdamW on the side stream
    bool tn_pending[2] = {false, false};
    // what the handle is: the late-fusion model (mmhip_create), or one tower under the fused CLS classifier head (mmhip_txt_create, mmhip_img_create)
    enum Kind { LATE, TEXT, IMAGE };
    Kind kind = LATE;
    bool is_late() const { return kind == LATE; }
    bool is_text() const { return kind == TEXT; }
    bool is_image() const { return kind == IMAGE; }
    // text-only handle (mmhip_txt_create): the text tower and the fused CLS classifier head alone -- no image tower, pooler, ITC / ITM or fusion head,
    // none of their workspace; parameters under the reference's text_only.py keys (bert_model.*, linear.*)
    std::string tm_prefix = "dual_encoder.text_model.";      // state-dict prefix of the text tower
    size_t lin_w = 0, lin_b = 0;                             // text-only classifier
    size_t tt_all = 0; bool has_tt = false;                  // the engine's clamped copy of the token type ids; the last forward was given some
                                                             // (has_tt is raised by txt_forward_impl alone: no late-fusion handle ever has it, so text_embed
                                                             // reads tt_all, which only a text-only workspace carves, on that handle kind only)
    // image-only handle (mmhip_img_create): the image tower, trainable, under the fused CLS classifier head -- parameters under the keys of HF
    // ViTForImageClassification (vit.*, classifier.*) in the trainable buffer, the tower's offsets in vit / v_*; no text tower, no frozen buffer
    std::vector<ImgAct> iact;
    size_t i_xfin = 0, i_cls = 0, i_clsln = 0, i_mean = 0, i_rstd = 0, i_dcls = 0, i_dclsx = 0, i_dclsx_p = 0;      // last stream; CLS rows around the final LayerNorm
    size_t i_dxs[3] = {0, 0, 0}, i_dxs_p[3] = {0, 0, 0};      // residual-stream gradients (+ their plane pairs): layer l reads [(l + 1) % 3], writes [l % 3]
    size_t i_set[2][4];        // per layer parity, read by the side stream: du, dqkv, d mid stream, its plane pair
    size_t i_dln = 0, i_dctx = 0, i_dpe = 0, i_epartial = 0;
    // The weight-gradient products reduce over the rows of a batch, B * P of them -- 3152 at the reference's batch size of 16, no multiple of the tile
    // kernels' 64-row slices.  Their operands therefore carry rows up to the next multiple of 64 (pad64), zero in both: the grouped tile kernel takes
    // every batch size.  Nothing ever writes those rows; they are cleared when the batch size changes (i_pad_B: the B they were cleared for).
    int i_pad_B = 0;
    static size_t pad64(size_t rows) { return (rows + 63) & ~(size_t)63; }
    int nl() const { return is_image() ? cfg.layers_img : cfg.layers_txt; }                 // layers with a backward stage
    const std::vector<LayerOff>& lay() const { return is_image() ? vit : txt; }
    const std::vector<LayerW16>& lay_w16() const { return is_image() ? vit_w16 : txt_w16; }
    int cls_only = -1;         // -1 = read MMHIP_CLS_ONLY on first use; 1: the last text layer runs its post-attention part on CLS rows only
    bool cls_compact = false;  // state of the last forward
    int overlap = -1;          // -1 = read MMHIP_OVERLAP on first use
    // CU partition of the forward (MMHIP_PART="txt,vit", e.g. "96,160"; read once): while both towers run side by side their big GEMMs are
    // persistent 256 x 256-tile launches of at most part[0] (text) / part[1] (image) workgroups.  A workgroup of that kernel holds a CU
    // (128 KB of LDS), so the two launches split the chip 96 / 160 without CU masks, each tower's GEMMs see a fixed machine (8192 rows x
    // 2304 / 768 / 3072 columns = 288 / 96 / 384 tiles = 3 / 1 / 4 rounds of 96; 12608 rows = 450 / 150 / 600 tiles = 2.8 / 0.94 / 3.75 rounds
    // of 160) instead of racing for CUs launch by launch.  cur_part: the caps of the forward being enqueued (0 = off).
    int part[2] = {-1, -1}, cur_part[2] = {0, 0}; bool part_auto = false;
    // mmhip_step_spans: timing events at the phase ends of the last forward / train step (0 fork, 1 image tower end, 2 text tower end,
    // 3 forward end, 4 backward end, 5 step end); recorded only while enabled
    int spans_on = 0; hipEvent_t span_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; bool span_set[6] = {false, false, false, false, false, false};
    int span(int i, hipStream_t s) {
        if (!spans_on) return 0;
        if (!span_ev[i]) { hipError_t r = hipEventCreate(&span_ev[i]); if (r != hipSuccess) return (int)r; }
        hipError_t r = hipEventRecord(span_ev[i], s);
        span_set[i] = r == hipSuccess;
        return (int)r;
    }
    // GEMM timing ----------------------------------------------------------------------
    int timing = 0;            // 0 off, 1 = events around every NT GEMM with the side streams on, 2 = side streams off
    struct Ev { hipEvent_t a, b; double flops; int M, N, K, flags, tile, cus; };      // cus: workgroup cap of a partitioned launch (0 = whole chip)
    std::vector<Ev> evs; size_t ev_used = 0;

    template <typename U> U* wsp(size_t off) const { return reinterpret_cast<U*>(ws + off); }
    int dt() const { return cfg.dtype; }
    // image tower geometry: its own width for CLIP-ViT-L/14 (BASELINE config 4), the text tower's otherwise
    bool clip() const { return cfg.img_kind == MMHIP_IMG_CLIP; }
    // BEiT tower (HF BeitModel, MMHIP_IMG_BEIT): no position embeddings, a relative position bias per layer and head inside the attention, layer
    // scale (folded into the 16-bit operand copies at refresh), a mean-pool pooler, and stochastic depth that the reference leaves on in train mode
    bool beit() const { return cfg.img_kind == MMHIP_IMG_BEIT; }
    std::vector<BeitWs> beit_ws;
    size_t beit_fold = 0;        // refresh scratch, fp32 [Hv, Iv]: a weight with its layer scale folded in, before the cast
    size_t beit_branch = 0;      // drop path: a residual branch [Mv, Hv] before its per-post scale is added to the stream
    float drop_path = 0.f;       // mmhip_set_drop_path: the last layer's drop probability; layer l takes linspace(0, rate, L)[l]
    int window() const { return cfg.image / cfg.patch; }
    int ldb() const { return (P() + 3) & ~3; }          // row stride of the bias image: a lane's four consecutive keys are one aligned 16-byte load
    float drop_path_p(int l) const {
        const int L = cfg.layers_img;
        return (train_mode && drop_path > 0.f && L > 1) ? drop_path * (float)l / (float)(L - 1) : 0.f;
    }
    bool aspect() const { return cfg.fusion == MMHIP_FUSION_ASPECT; }
    int Hv() const { return cfg.hidden_img > 0 ? cfg.hidden_img : cfg.hidden; }
    int Iv() const { return cfg.inter_img > 0 ? cfg.inter_img : cfg.inter; }
    int heads_v() const { return cfg.heads_img > 0 ? cfg.heads_img : cfg.heads; }
    int P() const { return (cfg.image / cfg.patch) * (cfg.image / cfg.patch) + 1; }
    int Kp() const { return 3 * cfg.patch * cfg.patch; }                 // patch-embedding reduction length
    int Kpp() const { return (Kp() + 63) / 64 * 64; }                    // ... padded to the GEMM's k-step (588 -> 640 for 14 x 14)
    size_t v_pre_ln_w = 0, v_pre_ln_b = 0;                               // CLIP pre_layrnorm
    // f16 activations: gradients inside the text tower are carried multiplied by gscale() (range, not precision) and
    // every fp32 parameter gradient is written multiplied by 1 / gscale(); bf16 needs none
    float gscale() const { return cfg.loss_scale > 0.f ? cfg.loss_scale : (cfg.dtype == MMHIP_F16 ? 1024.f : 1.f); }
    size_t esz() const { return cfg.dtype == MMHIP_BF16X3 ? 4 : 2; }
};

namespace {

// ------------------------------------------------------------------------------------------------ layout
// One transformer layer's 16 parameters, per family: {key suffix, the LayerOff slot the row sets (none: key / value follow query, the fused QKV
// operand reads the three as one [3H, H] block), shape}.  add_layer walks a table in its own order, so the table IS the layout of the layer.
enum class Shape { HH, H, IH, I, HI,
                   REL,      // BEiT: [(2W-1)^2 + 3, heads] relative position bias table
                   PAD };    // H unnamed elements: no parameter, never in mmhip_param_info_at (BEiT: the key bias HF does not have, zero-filled at refresh)
struct LayerKey { const char* suffix; size_t LayerOff::*slot; Shape shape; };
struct LayerKeys { const char* stem; LayerKey rows[20]; };      // rows past the last one have no suffix
// BERT / XLM-R text layer (post-LN)
const LayerKeys BERT_LAYER = {"encoder.layer.", {
    {"attention.self.query.weight", &LayerOff::qkv_w, Shape::HH}, {"attention.self.key.weight", nullptr, Shape::HH},
    {"attention.self.value.weight", nullptr, Shape::HH}, {"attention.self.query.bias", &LayerOff::qkv_b, Shape::H},
    {"attention.self.key.bias", nullptr, Shape::H}, {"attention.self.value.bias", nullptr, Shape::H},
    {"attention.output.dense.weight", &LayerOff::ao_w, Shape::HH}, {"attention.output.dense.bias", &LayerOff::ao_b, Shape::H},
    {"attention.output.LayerNorm.weight", &LayerOff::ln1_w, Shape::H}, {"attention.output.LayerNorm.bias", &LayerOff::ln1_b, Shape::H},
    {"intermediate.dense.weight", &LayerOff::fc1_w, Shape::IH}, {"intermediate.dense.bias", &LayerOff::fc1_b, Shape::I},
    {"output.dense.weight", &LayerOff::fc2_w, Shape::HI}, {"output.dense.bias", &LayerOff::fc2_b, Shape::H},
    {"output.LayerNorm.weight", &LayerOff::ln2_w, Shape::H}, {"output.LayerNorm.bias", &LayerOff::ln2_b, Shape::H}}};
// CLIP vision layer, transformers 4.25.1 keys (CLIPVisionModel wraps the transformer as `.vision_model`):
// HF:models/clip/modeling_clip.py (CLIPEncoderLayer: pre-LN, quick-GELU MLP)
const LayerKeys CLIP_LAYER = {"encoder.layers.", {
    {"self_attn.q_proj.weight", &LayerOff::qkv_w, Shape::HH}, {"self_attn.k_proj.weight", nullptr, Shape::HH},
    {"self_attn.v_proj.weight", nullptr, Shape::HH}, {"self_attn.q_proj.bias", &LayerOff::qkv_b, Shape::H},
    {"self_attn.k_proj.bias", nullptr, Shape::H}, {"self_attn.v_proj.bias", nullptr, Shape::H},
    {"self_attn.out_proj.weight", &LayerOff::ao_w, Shape::HH}, {"self_attn.out_proj.bias", &LayerOff::ao_b, Shape::H},
    {"layer_norm1.weight", &LayerOff::ln1_w, Shape::H}, {"layer_norm1.bias", &LayerOff::ln1_b, Shape::H},
    {"mlp.fc1.weight", &LayerOff::fc1_w, Shape::IH}, {"mlp.fc1.bias", &LayerOff::fc1_b, Shape::I},
    {"mlp.fc2.weight", &LayerOff::fc2_w, Shape::HI}, {"mlp.fc2.bias", &LayerOff::fc2_b, Shape::H},
    {"layer_norm2.weight", &LayerOff::ln2_w, Shape::H}, {"layer_norm2.bias", &LayerOff::ln2_b, Shape::H}}};
// HF ViTLayer (the frozen tower of the dual encoder; the trainable one of the image-only model): its two LayerNorms come last
const LayerKeys VIT_LAYER = {"encoder.layer.", {
    {"attention.attention.query.weight", &LayerOff::qkv_w, Shape::HH}, {"attention.attention.key.weight", nullptr, Shape::HH},
    {"attention.attention.value.weight", nullptr, Shape::HH}, {"attention.attention.query.bias", &LayerOff::qkv_b, Shape::H},
    {"attention.attention.key.bias", nullptr, Shape::H}, {"attention.attention.value.bias", nullptr, Shape::H},
    {"attention.output.dense.weight", &LayerOff::ao_w, Shape::HH}, {"attention.output.dense.bias", &LayerOff::ao_b, Shape::H},
    {"intermediate.dense.weight", &LayerOff::fc1_w, Shape::IH}, {"intermediate.dense.bias", &LayerOff::fc1_b, Shape::I},
    {"output.dense.weight", &LayerOff::fc2_w, Shape::HI}, {"output.dense.bias", &LayerOff::fc2_b, Shape::H},
    {"layernorm_before.weight", &LayerOff::ln1_w, Shape::H}, {"layernorm_before.bias", &LayerOff::ln1_b, Shape::H},
    {"layernorm_after.weight", &LayerOff::ln2_w, Shape::H}, {"layernorm_after.bias", &LayerOff::ln2_b, Shape::H}}};
// HF BeitLayer, transformers 4.25.1 keys: the key projection has no bias -- the packed QKV GEMM reads one [3H] bias block, so an unnamed zero slot
// stands where it would be -- a relative position bias table per layer (use_shared_relative_position_bias = False), two layer scales
const LayerKeys BEIT_LAYER = {"encoder.layer.", {
    {"attention.attention.query.weight", &LayerOff::qkv_w, Shape::HH}, {"attention.attention.key.weight", nullptr, Shape::HH},
    {"attention.attention.value.weight", nullptr, Shape::HH}, {"attention.attention.query.bias", &LayerOff::qkv_b, Shape::H},
    {"", nullptr, Shape::PAD}, {"attention.attention.value.bias", nullptr, Shape::H},
    {"attention.attention.relative_position_bias.relative_position_bias_table", &LayerOff::rel_table, Shape::REL},
    {"attention.output.dense.weight", &LayerOff::ao_w, Shape::HH}, {"attention.output.dense.bias", &LayerOff::ao_b, Shape::H},
    {"intermediate.dense.weight", &LayerOff::fc1_w, Shape::IH}, {"intermediate.dense.bias", &LayerOff::fc1_b, Shape::I},
    {"output.dense.weight", &LayerOff::fc2_w, Shape::HI}, {"output.dense.bias", &LayerOff::fc2_b, Shape::H},
    {"lambda_1", &LayerOff::lambda1, Shape::H}, {"lambda_2", &LayerOff::lambda2, Shape::H},
    {"layernorm_before.weight", &LayerOff::ln1_w, Shape::H}, {"layernorm_before.bias", &LayerOff::ln1_b, Shape::H},
    {"layernorm_after.weight", &LayerOff::ln2_w, Shape::H}, {"layernorm_after.bias", &LayerOff::ln2_b, Shape::H}}};
// layer l of a tower under `prefix`, in buffer `buf` and group `g`; rel_rows / heads: the shape of a Shape::REL row
void add_layer(ParamTable& b, const LayerKeys& keys, const std::string& prefix, int l, int buf, int g, int H, int I, LayerOff& o, int rel_rows = 0, int heads = 0) {
    const std::string p = prefix + keys.stem + std::to_string(l) + ".";
    o.begin = b.off[buf];
    for (const LayerKey& k : keys.rows) {
        if (!k.suffix) break;
        size_t at = 0;
        switch (k.shape) {
            case Shape::REL: at = b.add(p + k.suffix, buf, g, {rel_rows, heads}); break;
            case Shape::PAD: at = b.off[buf]; b.off[buf] += (size_t)H; break;          // (H % 4 == 0: the next tensor stays 16-byte aligned)
            case Shape::HH: at = b.add(p + k.suffix, buf, g, {H, H}); break;
            case Shape::H: at = b.add(p + k.suffix, buf, g, {H}); break;
            case Shape::IH: at = b.add(p + k.suffix, buf, g, {I, H}); break;
            case Shape::I: at = b.add(p + k.suffix, buf, g, {I}); break;
            case Shape::HI: at = b.add(p + k.suffix, buf, g, {H, I}); break;
        }
        if (k.slot) o.*k.slot = at;
    }
    o.end = b.off[buf];
}

// text layers last -> first, then the embeddings: the tail of the trainable buffer in both layouts (the word table closes it)
void add_text_layers_and_embeddings(mmhip_engine& e, ParamTable& b) {
    const mmhip_config& c = e.cfg;
    const int H = c.hidden;
    e.txt.resize(c.layers_txt);
    for (int l = c.layers_txt - 1; l >= 0; --l) add_layer(b, BERT_LAYER, e.tm_prefix, l, 1, MMHIP_G_ALWAYS, H, c.inter, e.txt[l]);
    const std::string tm = e.tm_prefix + "embeddings.";
    e.emb_begin = b.off[1];
    e.t_eln_w = b.add(tm + "LayerNorm.weight", 1, MMHIP_G_ALWAYS, {H});
    e.t_eln_b = b.add(tm + "LayerNorm.bias", 1, MMHIP_G_ALWAYS, {H});
    e.t_type = b.add(tm + "token_type_embeddings.weight", 1, MMHIP_G_ALWAYS, {c.type_vocab, H});
    e.t_pos = b.add(tm + "position_embeddings.weight", 1, MMHIP_G_ALWAYS, {c.max_pos, H});
    e.t_word = b.add(tm + "word_embeddings.weight", 1, MMHIP_G_ALWAYS, {c.vocab, H});
    e.emb_end = b.off[1];
}

void build_layout(mmhip_engine& e) {
    const mmhip_config& c = e.cfg;
    const int H = c.hidden, C = c.num_labels, E = c.proj_dim, P = e.P(), Hv = e.Hv();
    ParamTable b{e.params};
    // ---- frozen: vision tower (every dual_encoder parameter with 'vision' in its name, mm_late.py:67-69)
    e.vit.resize(c.layers_img);
    if (e.beit()) {
        // HF BeitModel (models/beit/modeling_beit.py) as microsoft/beit-base-patch16-224-pt22k-ft22k configures it: no position embeddings, no final
        // layernorm (Identity under mean pooling), the pooler is a LayerNorm over the mean of the patch tokens
        const std::string vm = "dual_encoder.vision_model.";
        const int W = e.window(), rel = (2 * W - 1) * (2 * W - 1) + 3;
        e.v_cls = b.add(vm + "embeddings.cls_token", 0, MMHIP_G_FROZEN, {1, 1, Hv});
        e.v_pos = 0;
        e.v_patch_w = b.add(vm + "embeddings.patch_embeddings.projection.weight", 0, MMHIP_G_FROZEN, {Hv, 3, c.patch, c.patch});
        e.v_patch_b = b.add(vm + "embeddings.patch_embeddings.projection.bias", 0, MMHIP_G_FROZEN, {Hv});
        for (int l = 0; l < c.layers_img; ++l) add_layer(b, BEIT_LAYER, vm, l, 0, MMHIP_G_FROZEN, Hv, e.Iv(), e.vit[l], rel, e.heads_v());
        e.v_ln_w = b.add(vm + "pooler.layernorm.weight", 0, MMHIP_G_FROZEN, {Hv});
        e.v_ln_b = b.add(vm + "pooler.layernorm.bias", 0, MMHIP_G_FROZEN, {Hv});
        e.v_pool_w = e.v_pool_b = 0;
    } else if (e.clip()) {
        // HF CLIPVisionTransformer (models/clip/modeling_clip.py): class_embedding [Hv], bias-free patch conv, learned positions,
        // pre_layrnorm, pre-LN layers, post_layernorm on the pooled CLS row only
        const std::string vm = "dual_encoder.vision_model.vision_model.";
        e.v_cls = b.add(vm + "embeddings.class_embedding", 0, MMHIP_G_FROZEN, {Hv});
        e.v_patch_w = b.add(vm + "embeddings.patch_embedding.weight", 0, MMHIP_G_FROZEN, {Hv, 3, c.patch, c.patch});
        e.v_patch_b = 0;
        e.v_pos = b.add(vm + "embeddings.position_embedding.weight", 0, MMHIP_G_FROZEN, {P, Hv});
        e.v_pre_ln_w = b.add(vm + "pre_layrnorm.weight", 0, MMHIP_G_FROZEN, {Hv});
        e.v_pre_ln_b = b.add(vm + "pre_layrnorm.bias", 0, MMHIP_G_FROZEN, {Hv});
        for (int l = 0; l < c.layers_img; ++l) add_layer(b, CLIP_LAYER, vm, l, 0, MMHIP_G_FROZEN, Hv, e.Iv(), e.vit[l]);
        e.v_ln_w = b.add(vm + "post_layernorm.weight", 0, MMHIP_G_FROZEN, {Hv});
        e.v_ln_b = b.add(vm + "post_layernorm.bias", 0, MMHIP_G_FROZEN, {Hv});
        e.v_pool_w = e.v_pool_b = 0;
    } else {
        const std::string vm = "dual_encoder.vision_model.";
        e.v_cls = b.add(vm + "embeddings.cls_token", 0, MMHIP_G_FROZEN, {1, 1, Hv});
        e.v_pos = b.add(vm + "embeddings.position_embeddings", 0, MMHIP_G_FROZEN, {1, P, Hv});
        e.v_patch_w = b.add(vm + "embeddings.patch_embeddings.projection.weight", 0, MMHIP_G_FROZEN, {Hv, 3, c.patch, c.patch});
        e.v_patch_b = b.add(vm + "embeddings.patch_embeddings.projection.bias", 0, MMHIP_G_FROZEN, {Hv});
        for (int l = 0; l < c.layers_img; ++l) add_layer(b, VIT_LAYER, vm, l, 0, MMHIP_G_FROZEN, Hv, e.Iv(), e.vit[l]);
        e.v_ln_w = b.add(vm + "layernorm.weight", 0, MMHIP_G_FROZEN, {Hv});
        e.v_ln_b = b.add(vm + "layernorm.bias", 0, MMHIP_G_FROZEN, {Hv});
        e.v_pool_w = b.add(vm + "pooler.dense.weight", 0, MMHIP_G_FROZEN, {Hv, Hv});
        e.v_pool_b = b.add(vm + "pooler.dense.bias", 0, MMHIP_G_FROZEN, {Hv});
    }
    // ---- trainable, ordered [never | ITC | ITM | fusion-attention | always: heads, layers last->first, embeddings]
    // An aspect-att handle (MMHIP_FUSION_ASPECT) has its own order: fc_Q / fc_K / fc_V and linear_fusion join the never group in front of the heads'
    // range (mm_late.py:115-131 reads none of them), aspectattention.* leaves it for the always group, and the text pooler -- consumed by the fusion
    // itself, not by ITC alone -- is tagged always.  Concat / attention handles keep every name, offset and group as they were.
    const bool aspect = e.aspect();
    for (const char* n : {"aspectattention", "linear_iadds", "linear_gmu_t", "linear_gmu_v"}) {
        if (aspect && !strcmp(n, "aspectattention")) continue;
        const int out = !strcmp(n, "aspectattention") ? 1 : (!strcmp(n, "linear_iadds") ? 2 : 2 * H);
        b.add(std::string(n) + ".weight", 1, MMHIP_G_NEVER, {out, H});
        b.add(std::string(n) + ".bias", 1, MMHIP_G_NEVER, {out});
    }
    auto add_attention_and_fusion = [&](int g_att, int g_fus) {
        e.fq_w = b.add("fc_Q.weight", 1, g_att, {H, H});
        e.fq_b = b.add("fc_Q.bias", 1, g_att, {H});
        e.fk_w = b.add("fc_K.weight", 1, g_att, {H, H});
        e.fk_b = b.add("fc_K.bias", 1, g_att, {H});
        e.fv_w = b.add("fc_V.weight", 1, g_att, {H, H});
        e.fv_b = b.add("fc_V.bias", 1, g_att, {H});
        // 'concat' takes [x_t CLS | x_v CLS]: H + Hv wide (the reference hard-wires 768 + 768, models/config.py:82-84, mm_late.py:81)
        e.fus_w = b.add("linear_fusion.weight", 1, g_fus, {H, H + Hv});
        e.fus_b = b.add("linear_fusion.bias", 1, g_fus, {H});
    };
    if (aspect) add_attention_and_fusion(MMHIP_G_NEVER, MMHIP_G_NEVER);
    e.heads_begin = b.off[1];
    e.logit_scale = b.add("dual_encoder.logit_scale", 1, MMHIP_G_ITC, {});
    e.vproj_w = b.add("dual_encoder.visual_projection.weight", 1, MMHIP_G_ITC, {E, Hv});
    e.tproj_w = b.add("dual_encoder.text_projection.weight", 1, MMHIP_G_ITC, {E, H});
    e.t_pool_w = b.add("dual_encoder.text_model.pooler.dense.weight", 1, aspect ? MMHIP_G_ALWAYS : MMHIP_G_ITC, {H, H});
    e.t_pool_b = b.add("dual_encoder.text_model.pooler.dense.bias", 1, aspect ? MMHIP_G_ALWAYS : MMHIP_G_ITC, {H});
    e.tim_w = b.add("linear_tim.weight", 1, MMHIP_G_ITM, {2, H});
    e.tim_b = b.add("linear_tim.bias", 1, MMHIP_G_ITM, {2});
    if (!aspect) add_attention_and_fusion(MMHIP_G_FUSION_ATT, MMHIP_G_ALWAYS);
    if (aspect) {
        e.asp_w = b.add("aspectattention.weight", 1, MMHIP_G_ALWAYS, {1, H});
        e.asp_b = b.add("aspectattention.bias", 1, MMHIP_G_ALWAYS, {1});
    }
    e.cls_w = b.add("linear_cls.weight", 1, MMHIP_G_ALWAYS, {C, H});
    e.cls_b = b.add("linear_cls.bias", 1, MMHIP_G_ALWAYS, {C});
    e.heads_end = b.off[1];
    add_text_layers_and_embeddings(e, b);
    e.n_frozen = b.off[0];
    e.n_train = b.off[1];
}

// the reference's text_only.py modules (BERT / BERNICE): bert_model.* + linear.*.  They classify last_hidden[:, 0, :]; the pooler is computed there
// and never consumed, so its parameters exist (checkpoint keys), sit in MMHIP_G_NEVER, get no gradient and no optimizer step.
// Order: [never: pooler | always: classifier, layers last -> first, embeddings]
void build_layout_txt(mmhip_engine& e) {
    const mmhip_config& c = e.cfg;
    const int H = c.hidden, C = c.num_labels;
    ParamTable b{e.params};
    e.t_pool_w = b.add(e.tm_prefix + "pooler.dense.weight", 1, MMHIP_G_NEVER, {H, H});
    e.t_pool_b = b.add(e.tm_prefix + "pooler.dense.bias", 1, MMHIP_G_NEVER, {H});
    e.heads_begin = b.off[1];
    e.lin_w = b.add("linear.weight", 1, MMHIP_G_ALWAYS, {C, H});
    e.lin_b = b.add("linear.bias", 1, MMHIP_G_ALWAYS, {C});
    e.heads_end = b.off[1];
    add_text_layers_and_embeddings(e, b);
    e.n_frozen = 0;
    e.n_train = b.off[1];
}

// HF ViTForImageClassification (the reference's image_only.py `vit` branch): no pooler; every parameter trains in one AdamW group.
// Order: [classifier, vit.layernorm | layers last -> first | embeddings: patch weight, patch bias, position_embeddings, cls_token] -- the backward
// finishes these address ranges in this order
void build_layout_img(mmhip_engine& e) {
    const mmhip_config& c = e.cfg;
    const int H = e.Hv(), C = c.num_labels, P = e.P(), g = MMHIP_G_ALWAYS;
    ParamTable b{e.params};
    e.heads_begin = b.off[1];
    e.lin_w = b.add("classifier.weight", 1, g, {C, H});
    e.lin_b = b.add("classifier.bias", 1, g, {C});
    e.v_ln_w = b.add("vit.layernorm.weight", 1, g, {H});
    e.v_ln_b = b.add("vit.layernorm.bias", 1, g, {H});
    e.heads_end = b.off[1];
    e.vit.resize(c.layers_img);
    for (int l = c.layers_img - 1; l >= 0; --l) add_layer(b, VIT_LAYER, "vit.", l, 1, g, H, e.Iv(), e.vit[l]);
    e.emb_begin = b.off[1];
    e.v_patch_w = b.add("vit.embeddings.patch_embeddings.projection.weight", 1, g, {H, 3, c.patch, c.patch});
    e.v_patch_b = b.add("vit.embeddings.patch_embeddings.projection.bias", 1, g, {H});
    e.v_pos = b.add("vit.embeddings.position_embeddings", 1, g, {1, P, H});
    e.v_cls = b.add("vit.embeddings.cls_token", 1, g, {1, 1, H});
    e.emb_end = b.off[1];
    e.v_pool_w = e.v_pool_b = 0;
    e.n_frozen = 0;
    e.n_train = b.off[1];
}

// ------------------------------------------------------------------------------------------------ workspace sizing shared by every handle kind
// 16-bit (parity mode: Z = 4) GEMM operand copies of n layers of a tower, H wide with an I-wide MLP; transposed: the copies the backward reads too
void carve_w16(Carver& w, std::vector<LayerW16>& v, int n, bool transposed, size_t H, size_t I, size_t Z) {
    v.resize(n);
    for (auto& L : v) {
        L.qkv = w.take(3 * H * H * Z); L.ao = w.take(H * H * Z); L.fc1 = w.take(I * H * Z); L.fc2 = w.take(H * I * Z);
        if (transposed) { L.qkvT = w.take(3 * H * H * Z); L.aoT = w.take(H * H * Z); L.fc1T = w.take(I * H * Z); L.fc2T = w.take(H * I * Z); }
    }
}
// fp32 scratch of the split-K path of the <= 128-row GEMMs of a tower: what run_gemm may hand to launch_nt_splitk
size_t splitk_floats(size_t H, size_t I) { return (size_t)(I / 384 + 1) * 128 * (size_t)(I > 3 * H ? I : 3 * H); }
// parity mode without plane pairs: split planes of the operands of one GEMM call at a time per stream (x3.hip) -- the widest NT problem of a
// tower's layer over M rows, and the four weight-gradient problems of a layer together
size_t x3_nt_bytes(size_t M, size_t H, size_t I) {
    size_t b = 0;
    const size_t nk[5][2] = {{3 * H, H}, {H, H}, {I, H}, {H, I}, {H, 3 * H}};
    for (auto& q : nk) { const size_t v = x3_nt_scratch_bytes((int)M, (int)q[0], (int)q[1]); if (v > b) b = v; }
    return b;
}
size_t x3_tn_bytes(size_t M, size_t H, size_t I) {
    return x3_tn_scratch_bytes((int)M, (int)H, (int)I) + x3_tn_scratch_bytes((int)M, (int)I, (int)H) + x3_tn_scratch_bytes((int)M, (int)(3 * H), (int)H) +
           x3_tn_scratch_bytes((int)M, (int)H, (int)H);
}

// the image tower's share alone: operand copies with transposes, the activations a pre-LN backward needs, its gradient temporaries, the head's words
void build_workspace_img(mmhip_engine& e) {
    const mmhip_config& c = e.cfg;
    const size_t H = e.Hv(), I = e.Iv(), C = c.num_labels, Bm = c.max_posts, P = e.P(), Kpp = e.Kpp(), Z = e.esz();
    const size_t Mv = mmhip_engine::pad64(Bm * P), Mp = mmhip_engine::pad64(Bm * (P - 1));      // rows of every token / patch tensor: padded (i_pad_B)
    Carver w;
    carve_w16(w, e.vit_w16, c.layers_img, true, H, I, Z);
    e.patch_w16 = w.take(H * Kpp * Z);
    e.v_patches = w.take(Mp * Kpp * Z); e.v_pe = w.take(Mp * H * Z);
    e.iact.resize(c.layers_img);
    for (auto& a : e.iact) {
        a.x_in = w.take(Mv * H * Z); a.ln1 = w.take(Mv * H * Z); a.qkv = w.take(Mv * 3 * H * Z); a.ctx = w.take(Mv * H * Z);
        a.lse = w.take(Bm * e.heads_v() * P * 4);
        a.x_mid = w.take(Mv * H * Z); a.ln2 = w.take(Mv * H * Z); a.u = w.take(Mv * I * Z); a.h = w.take(Mv * I * Z);
        a.mean1 = w.take(Mv * 4); a.rstd1 = w.take(Mv * 4); a.mean2 = w.take(Mv * 4); a.rstd2 = w.take(Mv * 4);
    }
    e.i_xfin = w.take(Mv * H * Z);
    e.i_cls = w.take(Bm * H * Z); e.i_clsln = w.take(Bm * H * Z); e.i_mean = w.take(Bm * 4); e.i_rstd = w.take(Bm * 4);
    e.i_dcls = w.take(Bm * H * Z); e.i_dclsx = w.take(Bm * H * Z);
    if (e.px) e.i_dclsx_p = w.take(Bm * H * Z);
    for (int i = 0; i < 3; ++i) {
        e.i_dxs[i] = w.take(Mv * H * Z);
        if (e.px) e.i_dxs_p[i] = w.take(Mv * H * Z);
    }
    for (int i = 0; i < 2; ++i) {
        e.i_set[i][0] = w.take(Mv * I * Z); e.i_set[i][1] = w.take(Mv * 3 * H * Z); e.i_set[i][2] = w.take(Mv * H * Z);
        e.i_set[i][3] = e.px ? w.take(Mv * H * Z) : 0;
        for (int j = 0; j < 2; ++j) e.g_lnp[i][j] = w.take(partial_floats_rows((int)Mv, (int)H, 2) * 4);
    }
    e.i_dln = w.take(Mv * H * Z); e.i_dctx = w.take(Mv * H * Z); e.i_dpe = w.take(Mp * H * Z);
    e.g_partial = w.take(partial_floats_rows((int)Bm, (int)H, 2) * 4);
    e.i_epartial = w.take(partial_floats_vit_embed((int)Bm, (int)P, (int)H) * 4);
    auto f = [&](size_t n) { return w.take(n * 4); };
    e.h_out_cls = f(Bm * C); e.h_d_out_cls = f(Bm * C); e.h_loss = f(8);
    e.splitk_ws = f(splitk_floats(H, I)); e.has_splitk = true;
    if (c.dtype == MMHIP_BF16X3 && !e.px) {
        // parity mode without plane pairs: split planes of one GEMM call at a time per stream -- the widest NT problem (the patch GEMM included),
        // the four weight-gradient problems of a layer together, or the patch weight's
        size_t b = x3_nt_scratch_bytes((int)Mp, (int)H, (int)Kpp);
        for (const size_t v : {x3_nt_bytes(Mv, H, I), x3_tn_bytes(Mv, H, I), x3_tn_scratch_bytes((int)Mp, (int)H, (int)Kpp)})
            if (v > b) b = v;
        e.x3_bytes[0] = e.x3_bytes[1] = b; e.x3_bytes[2] = 0;
        for (int i = 0; i < 2; ++i) e.x3_ws[i] = w.take(b);
    }
    e.ws_need = e.ws_base = w.off;
}

void build_workspace(mmhip_engine& e) {
    const mmhip_config& c = e.cfg;
    const size_t H = c.hidden, I = c.inter, E = c.proj_dim, C = c.num_labels;
    const size_t Bm = c.max_posts, Tm = c.max_text_len, P = e.P(), Hv = e.Hv(), Iv = e.Iv(), Kpp = e.Kpp();
    const bool mm = e.is_late();      // a text-only handle carves the text tower's share alone, for B (not 2 B: no ITM posts) rows of posts
    const size_t Bt = (mm ? 2 : 1) * Bm, Mt = Bt * Tm, Mv = Bm * P;
    const size_t Z = e.esz();      // bytes per activation / GEMM-operand element: 2 (bf16, f16) or 4 (bf16x3 parity mode)
    Carver w;
    carve_w16(w, e.vit_w16, mm ? c.layers_img : 0, false, Hv, Iv, Z);
    carve_w16(w, e.txt_w16, c.layers_txt, true, H, I, Z);
    if (mm) e.patch_w16 = w.take(Hv * Kpp * Z);
    else e.tt_all = w.take(Bt * Tm * 8);
    e.ids_all = w.take(Bt * Tm * 8); e.mask_all = w.take(Bt * Tm * 8); e.pos_ids = w.take(Bt * Tm * 4); e.maskbias = w.take(Bt * Tm * 4);
    e.x0 = w.take(Mt * H * Z); e.xhat_emb = w.take(Mt * H * Z); e.rstd_emb = w.take(Mt * 4);
    if (e.px) e.x0p = w.take(Mt * H * Z);
    e.tact.resize(c.layers_txt);
    for (auto& a : e.tact) {
        a.a1p = a.outp = 0;
        if (e.px) { a.a1p = w.take(Mt * H * Z); a.outp = w.take(Mt * H * Z); }
        a.qkv = w.take(Mt * 3 * H * Z); a.ctx = w.take(Mt * H * Z); a.pre1 = w.take(Mt * H * Z); a.a1 = w.take(Mt * H * Z);
        a.u = w.take(Mt * I * Z); a.h = w.take(Mt * I * Z); a.pre2 = w.take(Mt * H * Z); a.out = w.take(Mt * H * Z);
        a.mean1 = w.take(Mt * 4); a.rstd1 = w.take(Mt * 4); a.mean2 = w.take(Mt * 4); a.rstd2 = w.take(Mt * 4);
        a.lse = w.take(Bt * c.heads * Tm * 4);
    }
    if (mm) {
        e.v_patches = w.take(Bm * (P - 1) * Kpp * Z); e.v_pe = w.take(Bm * (P - 1) * Hv * Z);
        e.v_x = w.take(Mv * Hv * Z); e.v_ln = w.take(Mv * Hv * Z); e.v_qkv = w.take(Mv * 3 * Hv * Z); e.v_ctx = w.take(Mv * Hv * Z);
        e.v_h = w.take(Mv * Iv * Z); e.v_out = w.take(Mv * Hv * Z);
    }
    e.g_dx = w.take(Mt * H * Z); e.g_dx2 = w.take(Mt * H * Z); e.g_dpre = w.take(Mt * H * Z); e.g_ddrop = w.take(Mt * H * Z); e.g_dpre1 = w.take(Mt * H * Z); e.g_ddrop1 = w.take(Mt * H * Z);
    e.g_dqkv = w.take(Mt * 3 * H * Z); e.g_dctx = w.take(Mt * H * Z); e.g_du = w.take(Mt * I * Z);
    e.g_det_rows = w.take(Mt * H * 4);       // per-slot embedding gradient rows of the deterministic mode (MMHIP_DETERMINISTIC=1)
    e.g_set[0][0] = e.g_dpre; e.g_set[0][1] = e.g_ddrop; e.g_set[0][2] = e.g_du; e.g_set[0][3] = e.g_dpre1; e.g_set[0][4] = e.g_ddrop1; e.g_set[0][5] = e.g_dqkv;
    e.g_set[1][0] = w.take(Mt * H * Z); e.g_set[1][1] = w.take(Mt * H * Z); e.g_set[1][2] = w.take(Mt * I * Z);
    e.g_set[1][3] = w.take(Mt * H * Z); e.g_set[1][4] = w.take(Mt * H * Z); e.g_set[1][5] = w.take(Mt * 3 * H * Z);
    {
        size_t pf = partial_floats_rows((int)Mt, (int)H, 3), pc = partial_floats_colsum((int)Mt, (int)(3 * H > I ? 3 * H : I));
        // (a two-row token type table -- text-only BERT -- reduces a fourth vector: EmbedBwdArgs::type_rows)
        const size_t pe = partial_floats_embed((int)Bt, (int)Tm, (int)H) / 3 * (!mm && c.type_vocab > 1 ? 4 : 3);
        if (pe > pf) pf = pe;
        e.g_partial = w.take((pf > pc ? pf : pc) * 4);
        e.g_partial_side = w.take((pf > pc ? pf : pc) * 4);
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) e.g_lnp[i][j] = w.take(partial_floats_rows((int)Mt, (int)H, 2) * 4);
    }
    auto f = [&](size_t n) { return w.take(n * 4); };
    // the text tower's split-plane scratch: its widest NT problem, or the four weight-gradient problems of a layer together
    auto x3_txt = [&]() {
        const size_t tn = x3_tn_bytes(Mt, H, I), nt = x3_nt_bytes(Mt, H, I);
        return tn > nt ? tn : nt;
    };
    const bool x3_split = c.dtype == MMHIP_BF16X3 && !e.px;
    if (!mm) {          // the fused CLS head: logits, their gradient, the loss word, and d CLS rows when the last layer ran on full rows
        e.h_out_cls = f(Bm * C); e.h_d_out_cls = f(Bm * C); e.h_dxcls = f(Bm * H); e.h_loss = f(8);
        e.splitk_ws = f(splitk_floats(H, I)); e.has_splitk = true;
        if (x3_split) {
            e.x3_bytes[0] = e.x3_bytes[1] = x3_txt(); e.x3_bytes[2] = 0;
            for (int i = 0; i < 2; ++i) e.x3_ws[i] = w.take(e.x3_bytes[i]);
        }
        e.ws_need = e.ws_base = w.off;
        return;
    }
    e.h_vpool = f(Bm * Hv); e.h_tpool = f(Bm * H); e.h_txt_e = f(Bm * E); e.h_img_e = f(Bm * E); e.h_txt_n = f(Bm * E); e.h_img_n = f(Bm * E);
    e.h_txt_inv = f(Bm); e.h_img_inv = f(Bm); e.h_logits = f(Bm * Bm);
    e.h_q = f(Bt * H); e.h_qk = f(Bt * H); e.h_prob = f(Bt * P); e.h_xbar = f(Bt * H); e.h_z = f(Bt * (H + Hv)); e.h_feats = f(Bt * H);
    e.h_featd = f(Bm * H); e.h_out_cls = f(Bm * C); e.h_out_tim = f(Bm * 2);
    e.splitk_ws = f(splitk_floats(H, I)); e.has_splitk = true;
    e.splitk_ws_vit = f(splitk_floats(Hv, Iv));
    if (x3_split) {
        size_t vit = x3_nt_bytes(Mv, Hv, Iv);
        { const size_t pe = x3_nt_scratch_bytes((int)(Bm * (P - 1)), (int)Hv, (int)Kpp); if (pe > vit) vit = pe; }
        const size_t txt = x3_txt();
        e.x3_bytes[0] = txt > vit ? txt : vit; e.x3_bytes[1] = txt; e.x3_bytes[2] = vit;
        for (int i = 0; i < 3; ++i) e.x3_ws[i] = w.take(e.x3_bytes[i]);
    }
    e.h_d_out_cls = f(Bm * C); e.h_d_logits = f(Bm * Bm); e.h_d_out_tim = f(Bm * 2); e.h_dfeats = f(Bt * H); e.h_dpre = f(Bt * H);
    e.h_dz = f(Bt * (H + Hv)); e.h_dxcls = f(Bt * H); e.h_dxbar = f(Bt * H); e.h_dqk = f(Bt * H); e.h_dq = f(Bt * H);
    e.h_dtxt_e = f(Bm * E); e.h_dimg_e = f(Bm * E); e.h_dtpool = f(Bm * H); e.h_dprepool = f(Bm * H); e.h_loss = f(8);
    if (e.aspect()) { e.h_asp_w = f(Bm * 2); e.h_asp_e = f(Bm * 2); e.h_asp_partial = f(aspect_fusion_partial_floats((int)Bm, (int)H)); }
    if (e.beit()) {      // a BEiT handle alone: every other handle keeps its workspace size
        e.beit_ws.resize(c.layers_img);
        for (auto& L : e.beit_ws) { L.ao_b = f(Hv); L.fc2_b = f(Hv); L.bias = f((size_t)e.heads_v() * P * e.ldb()); }
        e.beit_fold = f(Hv * (Iv > Hv ? Iv : Hv));
        e.beit_branch = w.take(Mv * Hv * Z);
    }
    e.ws_need = e.ws_base = w.off;
}

inline uint32_t stream_attn(int l) { return 16 + 4 * l; }
inline uint32_t stream_attn_out(int l) { return 16 + 4 * l + 1; }
inline uint32_t stream_ffn_out(int l) { return 16 + 4 * l + 2; }

// ------------------------------------------------------------------------------------------------ GEMM helper
// forward GEMM of tower `which` (0 text, 1 image) under the CU partition: persistent 256 x 256 tiles on at most cur_part[which] workgroups
inline void part_gemm(const mmhip_engine& e, G& g, int which) {
    const int n = e.cur_part[which];
    if (n > 0 && !g.a.tile && g.a.M >= 2048 && g.a.N % 256 == 0 && g.a.K % 64 == 0 && (e.dt() == DT_BF16 || e.dt() == DT_F16)) g.tile(15).grid(n);
}
inline bool on_vit_stream(const mmhip_engine& e, hipStream_t s) { return e.side_vit[0] != nullptr && (s == e.side_vit[0] || s == e.side_vit[1]); }
// parity mode without plane pairs: the split-plane scratch of the stream a GEMM launch goes to -- the image tower's, the side stream's (only when the
// launch really is on it), else the caller's; {nullptr, 0} in every other mode
struct X3Scratch { char* ws; size_t bytes; };
inline X3Scratch x3_scratch(const mmhip_engine& e, hipStream_t s) {
    const int i = on_vit_stream(e, s) ? 2 : (e.side && s == e.side ? 1 : 0);
    return X3Scratch{e.x3_bytes[i] ? e.ws + e.x3_ws[i] : nullptr, e.x3_bytes[i]};
}
int run_gemm(mmhip_engine& e, G& g, hipStream_t s) {
    // GEMMs of <= 128 rows with K >= 1536 (the CLS-row GEMMs of the last text layer; a tiny image tower) are split along K
    // (gemm.hip launch_nt_splitk) through an fp32 scratch: the image tower's side stream has its own, every other stream shares the caller's
    {
        const bool on_vit = on_vit_stream(e, s);
        const size_t bound = on_vit ? splitk_floats(e.Hv(), e.Iv()) : splitk_floats(e.cfg.hidden, e.cfg.inter);
        if (e.has_splitk && g.a.M <= 128 && (size_t)(g.a.K / 384) * g.a.M * g.a.N <= bound)
            g.a.splitk_ws = e.wsp<float>(on_vit ? e.splitk_ws_vit : e.splitk_ws);
        if (e.x3_bytes[0]) {
            const X3Scratch x = x3_scratch(e, s);
            g.a.x3_ws = x.ws;
            g.a.x3_ws_bytes = x.bytes;
        }
    }
    if (e.timing) {
        if (e.ev_used == e.evs.size()) {
            mmhip_engine::Ev ev;
            CHECK_HIP(hipEventCreate(&ev.a));
            CHECK_HIP(hipEventCreate(&ev.b));
            e.evs.push_back(ev);
        }
        auto& ev = e.evs[e.ev_used++];
        ev.flops = 2.0 * g.a.M * (double)g.a.N * g.a.K;
        ev.M = g.a.M; ev.N = g.a.N; ev.K = g.a.K; ev.flags = g.a.flags; ev.tile = g.a.tile; ev.cus = g.a.grid;
        CHECK_HIP(hipEventRecord(ev.a, s));
        CHECK_HIP(launch_gemm_nt(g.a, e.dt(), s));
        CHECK_HIP(hipEventRecord(ev.b, s));
        return 0;
    }
    CHECK_HIP(launch_gemm_nt(g.a, e.dt(), s));
    return 0;
}

// ------------------------------------------------------------------------------------------------ side stream
int side_init(mmhip_engine& e) {
    if (e.overlap < 0) e.overlap = env_int("MMHIP_OVERLAP", 1);
    if (!e.overlap || e.side) return 0;
    // The side streams are borrowed from the process-wide pool (mmhip_common.h: pool_stream -- why they are not created per engine).
    // The forward's two towers race for the CUs: whichever chain is longer should not be the one that waits.  The image
    // tower gets the high-priority stream when it is the longer chain (plain batch: 34.9 vs 22.3 GF per post), the
    // normal one when the text pass is doubled by the ITM posts.  Measured same-box: -0.17 ms/step on config 2; the
    // same high priority on config 3 costs +0.38 ms.
    CHECK_HIP(pool_stream(POOL_SIDE, &e.side));
    CHECK_HIP(pool_stream(POOL_VIT, &e.side_vit[0]));
    CHECK_HIP(pool_stream(POOL_VIT_HI, &e.side_vit[1]));
    hipEvent_t* evs[9] = {&e.ev_fork, &e.ev_vit, &e.ev_ready[0], &e.ev_ready[1], &e.ev_tn[0], &e.ev_tn[1], &e.ev_layer[0], &e.ev_layer[1], &e.ev_opt};
    for (auto ev : evs) CHECK_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    return 0;
}
inline bool use_side(const mmhip_engine& e) { return e.overlap > 0 && e.side && e.timing != 2; }

// ------------------------------------------------------------------------------------------------ weights
int refresh_layer(mmhip_engine& e, const float* base, const LayerOff& o, const LayerW16& w, bool transposed, hipStream_t s, int H, int I) {
    CastMat m[4] = {{base + o.qkv_w, e.ws + w.qkv, transposed ? e.ws + w.qkvT : nullptr, 3 * H, H, 0},
                    {base + o.ao_w, e.ws + w.ao, transposed ? e.ws + w.aoT : nullptr, H, H, 0},
                    {base + o.fc1_w, e.ws + w.fc1, transposed ? e.ws + w.fc1T : nullptr, I, H, 0},
                    {base + o.fc2_w, e.ws + w.fc2, transposed ? e.ws + w.fc2T : nullptr, H, I, 0}};
    CHECK_HIP(launch_cast_group(m, 4, e.px ? DT_PAIR : e.dt(), s));
    return 0;
}
// BEiT layer l of the frozen tower.  The layer scales are folded into the operand copies in fp32, before the cast or the plane split:
// Wo' = diag(lambda_1) Wo, bo' = lambda_1 * bo, likewise lambda_2 into FC2 -- the residual epilogues then add lambda * branch as they are and the fp32
// masters stay as loaded.  The key bias slot is cleared, and the layer's bias table is expanded into its [heads][P][ldb] image.
int refresh_layer_beit(mmhip_engine& e, int l, hipStream_t s) {
    const float* F = e.frozen;
    const LayerOff& o = e.vit[l]; const LayerW16& w = e.vit_w16[l]; const BeitWs& bw = e.beit_ws[l];
    const int H = e.Hv(), I = e.Iv(), dt = e.px ? DT_PAIR : e.dt();
    float* fold = e.wsp<float>(e.beit_fold);
    CHECK_HIP(hipMemsetAsync(e.frozen + o.qkv_b + H, 0, (size_t)H * 4, s));
    CastMat m[2] = {{F + o.qkv_w, e.ws + w.qkv, nullptr, 3 * H, H, 0}, {F + o.fc1_w, e.ws + w.fc1, nullptr, I, H, 0}};
    CHECK_HIP(launch_cast_group(m, 2, dt, s));
    CHECK_HIP(launch_scale_rows_f32(F + o.ao_w, F + o.lambda1, fold, H, H, s));
    CastMat ao{fold, e.ws + w.ao, nullptr, H, H, 0};
    CHECK_HIP(launch_cast_group(&ao, 1, dt, s));
    CHECK_HIP(launch_scale_rows_f32(F + o.fc2_w, F + o.lambda2, fold, H, I, s));
    CastMat fc2{fold, e.ws + w.fc2, nullptr, H, I, 0};
    CHECK_HIP(launch_cast_group(&fc2, 1, dt, s));
    CHECK_HIP(launch_scale_rows_f32(F + o.ao_b, F + o.lambda1, e.wsp<float>(bw.ao_b), H, 1, s));
    CHECK_HIP(launch_scale_rows_f32(F + o.fc2_b, F + o.lambda2, e.wsp<float>(bw.fc2_b), H, 1, s));
    CHECK_HIP(launch_beit_bias_image(F + o.rel_table, e.heads_v(), e.window(), e.window(), e.wsp<float>(bw.bias), e.ldb(), s));
    return 0;
}
// patch-embedding weight [Hv, 3*p*p] of the tower whose parameters live in `base`, rows zero-padded to the GEMM's k-step (14 x 14 patches: 588 -> 640)
int refresh_patch(mmhip_engine& e, const float* base, hipStream_t s) {
    CHECK_HIP(launch_cast_pad(base + e.v_patch_w, e.ws + e.patch_w16, e.Hv(), e.Kp(), e.Kpp(), e.px ? DT_PAIR : e.dt(), s));
    return 0;
}

// ------------------------------------------------------------------------------------------------ forward pieces
// Every launch of a tower's forward is written once, here.  text_forward and vit_forward below are orderings of these pieces
// on the streams they name: a piece takes its stream from the caller and never chooses one (run_gemm picks its scratch by it), and every tower
// GEMM passes part_gemm (a no-op whenever the forward is not partitioned: cur_part = {0, 0}).
inline int run_gemm(mmhip_engine& e, G&& g, hipStream_t s) { return run_gemm(e, g, s); }

// text embeddings; opens a forward: MMHIP_CLS_ONLY is read on the engine's first one, and no layer has closed yet
int text_embed(mmhip_engine& e, hipStream_t s) {
    const mmhip_config& c = e.cfg;
    const float* W = e.train;
    EmbedArgs ea{};
    ea.ids = e.wsp<int64_t>(e.ids_all); ea.mask = e.wsp<int64_t>(e.mask_all);
    ea.word = W + e.t_word; ea.pos = W + e.t_pos; ea.type = W + e.t_type; ea.gamma = W + e.t_eln_w; ea.beta = W + e.t_eln_b;
    ea.x = e.ws + e.x0; ea.xhat = e.ws + e.xhat_emb; ea.rstd = e.wsp<float>(e.rstd_emb); ea.pos_ids = e.wsp<int>(e.pos_ids);
    ea.maskbias = e.wsp<float>(e.maskbias);
    ea.posts = e.Bt; ea.T = e.T; ea.H = c.hidden; ea.xlmr = c.txt_kind == MMHIP_TXT_XLMR; ea.pad_id = c.pad_id; ea.eps = c.ln_eps_txt;
    ea.drop = make_drop(c.p_hidden, e.seed, STREAM_EMBED, e.train_mode);
    if (e.has_tt) ea.type_ids = e.wsp<int64_t>(e.tt_all);
    embed_pair(ea, e.px, e.ws + e.x0p);
    CHECK_HIP(launch_embed_fwd(ea, e.dt(), s));
    if (e.cls_only < 0) e.cls_only = env_int("MMHIP_CLS_ONLY", 1);
    e.cls_compact = false;
    return 0;
}

// The forward launches of text layer l.  Its input is the layer below's output (the embeddings' for l = 0): x as the residual reads it, xg as the
// GEMMs read it (parity mode: its plane pair).
// Only the CLS row of the last layer's output is ever consumed (fusion query and pooler, mm_late.py:111,155-158): its attention needs query
// tile 0 only and everything after it runs on Bt rows (row stride T*H in the full tensors, compact [Bt, .] outputs).  Dropout indices keep
// the full-tensor numbering (row_mul = T).
struct TextLayer {
    mmhip_engine& e;
    const int l;
    const LayerOff& o; const LayerW16& w; const TextAct& a;
    const float* W;
    const int H, I, T, Bt, Mt;
    const bool px, tr, compact;
    const int Mr, rs, rmul;
    const char *x, *xg;
    TextLayer(mmhip_engine& e, int l)
        : e(e), l(l), o(e.txt[l]), w(e.txt_w16[l]), a(e.tact[l]), W(e.train), H(e.cfg.hidden), I(e.cfg.inter), T(e.T), Bt(e.Bt), Mt(e.Bt * e.T), px(e.px),
          tr(e.train_mode), compact(e.cls_only > 0 && l == e.cfg.layers_txt - 1), Mr(compact ? Bt : Mt), rs(compact ? T * H : H), rmul(compact ? T : 1),
          x(e.ws + (l ? e.tact[l - 1].out : e.x0)), xg(px ? e.ws + (l ? e.tact[l - 1].outp : e.x0p) : x) {}
    G part(G& g) const { part_gemm(e, g, 0); return g; }
    G qkv() const { return part(G(xg, H, e.ws + w.qkv, H, e.ws + a.qkv, 3 * H, Mt, 3 * H, H).bias(W + o.qkv_b).px_in(px).px_out(px)); }
    int attention(hipStream_t s) const {
        AttnArgs at = attn_args(e.ws + a.qkv, e.wsp<float>(e.maskbias), e.ws + a.ctx, e.wsp<float>(a.lse), Bt, T, e.cfg.heads, H,
                                make_drop(e.cfg.p_attn, e.seed, stream_attn(l), tr));
        attn_pair(at, px);
        at.q_tiles = compact ? 1 : 0;
        CHECK_HIP(launch_attn_fwd(at, e.dt(), s));
        return 0;
    }
    G attn_out() const {
        return part(G(e.ws + a.ctx, rs, e.ws + w.ao, H, e.ws + a.pre1, H, Mr, H, H)
                        .bias(W + o.ao_b).dropout(make_drop(e.cfg.p_hidden, e.seed, stream_attn_out(l), tr), rmul).residual(x, rs).px_in(px));
    }
    G fc1() const { return part(G(e.ws + (px ? a.a1p : a.a1), H, e.ws + w.fc1, H, e.ws + a.h, I, Mr, I, H).bias(W + o.fc1_b).aux(e.ws + a.u, I).gelu().px_in(px).px_out(px)); }
    G fc2() const {
        return part(G(e.ws + a.h, I, e.ws + w.fc2, I, e.ws + a.pre2, H, Mr, H, I)
                        .bias(W + o.fc2_b).dropout(make_drop(e.cfg.p_hidden, e.seed, stream_ffn_out(l), tr), rmul).residual(e.ws + a.a1, H).px_in(px));
    }
    int ln(size_t in, size_t out, size_t pair, size_t gamma, size_t beta, size_t mean, size_t rstd, hipStream_t s) const {
        LNArgs n{e.ws + in, e.ws + out, W + gamma, W + beta, e.wsp<float>(mean), e.wsp<float>(rstd), Mr, H, H, H, e.cfg.ln_eps_txt};
        ln_pair(n, px, e.ws + pair);
        CHECK_HIP(launch_layernorm_fwd(n, e.dt(), s));
        return 0;
    }
    int ln1(hipStream_t s) const { return ln(a.pre1, a.a1, a.a1p, o.ln1_w, o.ln1_b, a.mean1, a.rstd1, s); }
    // closes the layer: from here on the engine's last hidden state is this layer's output, compact if it ran on the CLS rows
    int ln2(hipStream_t s) const {
        CHECK_RC(ln(a.pre2, a.out, a.outp, o.ln2_w, o.ln2_b, a.mean2, a.rstd2, s));
        e.cls_compact = compact;
        return 0;
    }
};

// patchify, patch GEMM, [CLS | patches] + positions, and CLIP's pre_layrnorm (in place; HF:models/clip/modeling_clip.py CLIPVisionTransformer.forward)
int vit_embed(mmhip_engine& e, const float* pixels, hipStream_t s) {
    const mmhip_config& c = e.cfg;
    const int H = e.Hv(), B = e.B, P = e.P(), Kpp = e.Kpp(), dt = e.dt();
    const float* F = e.is_image() ? e.train : e.frozen;
    char* x0 = e.ws + (!e.is_image() ? e.v_x : (c.layers_img ? e.iact[0].x_in : e.i_xfin));
    CHECK_HIP(launch_patchify(pixels, e.ws + e.v_patches, B, c.image, c.patch, Kpp, e.px ? DT_PAIR : dt, s));
    G g(e.ws + e.v_patches, Kpp, e.ws + e.patch_w16, Kpp, e.ws + e.v_pe, H, B * (P - 1), H, Kpp);
    if (!e.clip()) g.bias(F + e.v_patch_b);           // CLIP's patch conv has no bias
    g.px_in(e.px);
    part_gemm(e, g, 1);
    CHECK_RC(run_gemm(e, g, s));
    CHECK_HIP(launch_vit_assemble(e.ws + e.v_pe, F + e.v_cls, e.beit() ? nullptr : F + e.v_pos, x0, B, P, H, dt, s));      // BEiT: no absolute positions
    if (e.clip()) {
        LNArgs ln{x0, x0, F + e.v_pre_ln_w, F + e.v_pre_ln_b, nullptr, nullptr, B * P, H, H, H, c.ln_eps_img};
        CHECK_HIP(launch_layernorm_fwd(ln, dt, s));
    }
    return 0;
}

// The forward launches of image layer l (pre-LN: HF ViTLayer / CLIPEncoderLayer), written once over a buffer set.  The frozen tower of the late-fusion
// model runs every layer on the SHARED set: the residual stream v_x in place, one LayerNorm / qkv / ctx / h buffer, nothing kept.  The trainable
// tower of the image-only model gives each layer its OWN set (ImgAct): LayerNorm writes mean / rstd, attention its log-sum-exp, FC1 its pre-activation,
// and the residual GEMMs write the next saved stream instead of in place.
struct ImageBufs {
    const float* W;                     // fp32 parameters (biases, LayerNorm)
    char *x_in, *x_mid, *x_out;         // residual stream before the layer, after the attention block, after the MLP
    char *ln1, *ln2, *qkv, *ctx, *h, *u;
    float *lse, *mean1, *rstd1, *mean2, *rstd2;
};
inline ImageBufs image_bufs_shared(const mmhip_engine& e) {
    char* x = e.ws + e.v_x;
    return ImageBufs{e.frozen, x, x, x, e.ws + e.v_ln, e.ws + e.v_ln, e.ws + e.v_qkv, e.ws + e.v_ctx, e.ws + e.v_h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
}
inline ImageBufs image_bufs_saved(const mmhip_engine& e, int l) {
    const ImgAct& a = e.iact[l];
    char* out = e.ws + (l + 1 < e.cfg.layers_img ? e.iact[l + 1].x_in : e.i_xfin);
    return ImageBufs{e.train, e.ws + a.x_in, e.ws + a.x_mid, out, e.ws + a.ln1, e.ws + a.ln2, e.ws + a.qkv, e.ws + a.ctx, e.ws + a.h, e.ws + a.u,
                     e.wsp<float>(a.lse), e.wsp<float>(a.mean1), e.wsp<float>(a.rstd1), e.wsp<float>(a.mean2), e.wsp<float>(a.rstd2)};
}
struct ImageLayer {
    const mmhip_engine& e;
    const LayerOff& o; const LayerW16& w;
    const ImageBufs b;
    const float* F;
    const int l, H, I, Mv;
    const bool px;
    ImageLayer(const mmhip_engine& e, int l) : ImageLayer(e, l, image_bufs_shared(e)) {}
    ImageLayer(const mmhip_engine& e, int l, const ImageBufs& b)
        : e(e), o(e.vit[l]), w(e.vit_w16[l]), b(b), F(b.W), l(l), H(e.Hv()), I(e.Iv()), Mv(e.B * e.P()), px(e.px) {}
    // BEiT: the residual GEMMs read the biases with the layer scale folded in (refresh_layer_beit)
    const float* ao_bias() const { return e.beit() ? e.wsp<float>(e.beit_ws[l].ao_b) : F + o.ao_b; }
    const float* fc2_bias() const { return e.beit() ? e.wsp<float>(e.beit_ws[l].fc2_b) : F + o.fc2_b; }
    G part(G& g) const { part_gemm(e, g, 1); return g; }
    int ln(const char* x, char* y, size_t gamma, size_t beta, float* mean, float* rstd, hipStream_t s) const {
        LNArgs n{x, y, F + gamma, F + beta, mean, rstd, Mv, H, H, H, e.cfg.ln_eps_img};
        ln_pair(n, px, y, true);          // only GEMMs read it: the pair alone
        CHECK_HIP(launch_layernorm_fwd(n, e.dt(), s));
        return 0;
    }
    int ln1(hipStream_t s) const { return ln(b.x_in, b.ln1, o.ln1_w, o.ln1_b, b.mean1, b.rstd1, s); }
    int ln2(hipStream_t s) const { return ln(b.x_mid, b.ln2, o.ln2_w, o.ln2_b, b.mean2, b.rstd2, s); }
    G qkv() const { return part(G(b.ln1, H, e.ws + w.qkv, H, b.qkv, 3 * H, Mv, 3 * H, H).bias(F + o.qkv_b).px_in(px).px_out(px)); }
    int attention(hipStream_t s) const {
        AttnArgs at = attn_args(b.qkv, nullptr, b.ctx, b.lse, e.B, e.P(), e.heads_v(), H);
        attn_pair(at, px);
        if (e.beit()) {          // the layer's relative position bias, expanded at refresh
            CHECK_HIP(launch_attn_fwd_bias(attn_bias(at, e.wsp<float>(e.beit_ws[l].bias), e.ldb()), e.dt(), s));
            return 0;
        }
        CHECK_HIP(launch_attn_fwd(at, e.dt(), s));
        return 0;
    }
    G attn_out() const { return part(G(b.ctx, H, e.ws + w.ao, H, b.x_mid, H, Mv, H, H).bias(ao_bias()).residual(b.x_in, H).px_in(px)); }
    G fc1() const {
        G g(b.ln2, H, e.ws + w.fc1, H, b.h, I, Mv, I, H);
        g.bias(F + o.fc1_b);
        if (b.u) g.aux(b.u, I);
        if (e.clip()) g.qgelu(); else g.gelu();
        return part(g.px_in(px).px_out(px));
    }
    G fc2() const { return part(G(b.h, I, e.ws + w.fc2, I, b.x_out, H, Mv, H, I).bias(fc2_bias()).residual(b.x_mid, H).px_in(px)); }
    // Stochastic depth (BEiT, train mode, p_l > 0; the shared buffer set: the stream is updated in place).  The residual GEMM writes the branch -- bias
    // and layer scale included -- to a scratch tensor instead of adding it, and one more launch adds keep_scale * branch to the posts the hash keeps.
    // One draw per (layer, branch, post): the element index is the post's row in the batch.
    static uint32_t stream_droppath(int l, int which) { return 0x1000u + 2u * (uint32_t)l + (uint32_t)which; }
    G branch(int which) const {          // 0: the attention block's, 1: the MLP's
        char* scratch = e.ws + e.beit_branch;
        G g = which == 0 ? G(b.ctx, H, e.ws + w.ao, H, scratch, H, Mv, H, H).bias(ao_bias()) : G(b.h, I, e.ws + w.fc2, I, scratch, H, Mv, H, I).bias(fc2_bias());
        return part(g.px_in(px));
    }
    int droppath_add(int which, float p, hipStream_t s) const {
        CHECK_HIP(launch_droppath_add(which == 0 ? b.x_mid : b.x_out, e.ws + e.beit_branch, e.B, e.P(), H, make_drop(p, e.seed, stream_droppath(l, which)), e.dt(), s));
        return 0;
    }
};

// closes the image tower: last hidden state in v_out, pooled feature in h_vpool
int vit_close(mmhip_engine& e, hipStream_t s) {
    const int H = e.Hv(), B = e.B, P = e.P(), Mv = B * P, dt = e.dt();
    const float* F = e.frozen;
    char* x = e.ws + e.v_x;
    if (e.beit()) {
        // last_hidden_state = the encoder output as it is (BeitModel.layernorm is Identity under mean pooling); pooler_output = LayerNorm(mean of the
        // patch tokens), no dense, no tanh   (BeitPooler.forward)
        CHECK_HIP(hipMemcpyAsync(e.ws + e.v_out, x, (size_t)Mv * H * e.esz(), hipMemcpyDeviceToDevice, s));
        CHECK_HIP(launch_patch_mean_ln(x, P, B, H, F + e.v_ln_w, F + e.v_ln_b, e.cfg.ln_eps_img, e.wsp<float>(e.h_vpool), dt, s));
        return 0;
    }
    if (e.clip()) {
        // last_hidden_state = the encoder output as it is; pooler_output = post_layernorm(CLS row)   (CLIPVisionTransformer.forward)
        CHECK_HIP(hipMemcpyAsync(e.ws + e.v_out, x, (size_t)Mv * H * e.esz(), hipMemcpyDeviceToDevice, s));
        CHECK_HIP(launch_gather_rows_f32(x, (size_t)P * H, e.wsp<float>(e.h_vpool), H, B, H, dt, s));
        LNArgs lnp{e.wsp<float>(e.h_vpool), e.wsp<float>(e.h_vpool), F + e.v_ln_w, F + e.v_ln_b, nullptr, nullptr, B, H, H, H, e.cfg.ln_eps_img};
        CHECK_HIP(launch_layernorm_fwd(lnp, DT_F32, s));
        return 0;
    }
    LNArgs lnf{x, e.ws + e.v_out, F + e.v_ln_w, F + e.v_ln_b, nullptr, nullptr, Mv, H, H, H, e.cfg.ln_eps_img};
    CHECK_HIP(launch_layernorm_fwd(lnf, dt, s));
    // pooler on the CLS rows (row stride P*H): tanh(dense(x[:,0]))
    SmallGemmArgs sp = small(e.ws + e.v_out, P * H, F + e.v_pool_w, H, F + e.v_pool_b, e.wsp<float>(e.h_vpool), H, B, H, H, ACT_TANH);
    CHECK_HIP(launch_small_nt(sp, dt, s));
    return 0;
}

// ------------------------------------------------------------------------------------------------ the towers' forward: orderings of the pieces
// embeddings and every image layer in order; saved: each layer on its own buffer set (the trainable tower), else all on the shared one
int image_layers_forward(mmhip_engine& e, const float* pixels, bool saved, hipStream_t s) {
    CHECK_RC(vit_embed(e, pixels, s));
    for (int l = 0; l < e.cfg.layers_img; ++l) {
        const ImageLayer v(e, l, saved ? image_bufs_saved(e, l) : image_bufs_shared(e));
        CHECK_RC(v.ln1(s));
        CHECK_RC(run_gemm(e, v.qkv(), s));
        CHECK_RC(v.attention(s));
        const float p_drop = !saved && e.beit() ? e.drop_path_p(l) : 0.f;      // > 0: BEiT's stochastic depth is on for this layer
        if (p_drop > 0.f) {
            CHECK_RC(run_gemm(e, v.branch(0), s));
            CHECK_RC(v.droppath_add(0, p_drop, s));
        } else {
            CHECK_RC(run_gemm(e, v.attn_out(), s));
        }
        CHECK_RC(v.ln2(s));
        CHECK_RC(run_gemm(e, v.fc1(), s));
        if (p_drop > 0.f) {
            CHECK_RC(run_gemm(e, v.branch(1), s));
            CHECK_RC(v.droppath_add(1, p_drop, s));
        } else {
            CHECK_RC(run_gemm(e, v.fc2(), s));
        }
    }
    return 0;
}
// the frozen tower of the late-fusion model
int vit_forward(mmhip_engine& e, const float* pixels, hipStream_t s) {
    CHECK_RC(image_layers_forward(e, pixels, false, s));
    return vit_close(e, s);
}

int text_forward(mmhip_engine& e, hipStream_t s) {
    CHECK_RC(text_embed(e, s));
    for (int l = 0; l < e.cfg.layers_txt; ++l) {
        const TextLayer t(e, l);
        CHECK_RC(run_gemm(e, t.qkv(), s));
        CHECK_RC(t.attention(s));
        CHECK_RC(run_gemm(e, t.attn_out(), s));
        CHECK_RC(t.ln1(s));
        CHECK_RC(run_gemm(e, t.fc1(), s));
        CHECK_RC(run_gemm(e, t.fc2(), s));
        CHECK_RC(t.ln2(s));
    }
    return 0;
}

// The split of the chip's 256 CUs between the two towers of this forward: both towers' big GEMMs run 256 x 256 tiles of K / 64 K-steps
// each, a launch of n tiles on c workgroups takes ceil(n / c) rounds, a round costs its K-steps plus a fixed prologue + epilogue share
// (in K-step units: 5, from the in-kernel stamps: 7.5 us of 29.5 at K = 768).  Pick the split (whole XCD-eighths: multiples of 8) that
// minimises the longer tower; partition only when the model says it beats both towers sharing every launch's tail.
void choose_partition(mmhip_engine& e) {
    const mmhip_config& c = e.cfg;
    const int H = c.hidden, I = c.inter, Hv = e.Hv(), Iv = e.Iv();
    if (H % 256 || I % 256 || Hv % 256 || Iv % 256 || c.layers_txt < 1 || c.layers_img < 1) return;
    const long Mt = (long)e.Bt * e.T, Mv = (long)e.B * e.P();
    if (Mt < 2048 || Mv < 2048) return;
    const long rt = (Mt + 255) / 256, rv = (Mv + 255) / 256;
    auto tower = [](long rows, int h, int inter, int layers, int cap) -> double {
        auto gemm = [&](int n, int k) { const long tiles = rows * (n / 256); return (double)((tiles + cap - 1) / cap) * (k / 64 + 5); };
        return layers * (gemm(3 * h, h) + gemm(h, h) + gemm(inter, h) + gemm(h, inter));
    };
    // Same-box A/B of the step (profiles/r03_step_ab.txt): the split pays where the image tower is clearly the longer one (CLIP-L/14 beside
    // 32 posts of text: 12.8 vs 13.2 ms), is neutral to -3 % at config 2 (12608 image rows beside 8192 text rows: 10.24-10.30 either way on two boxes, 10.0 vs 10.3 on a third) and LOSES
    // where the text tower is the longer one (config 3, 16384 text rows with ITM: 15.95 vs 15.3 ms) -- free sharing then fills the tails of
    // the short tower's launches with the long tower's workgroups, which a fixed split forbids.
    // (model costs, image / text: config 2 1.12, config 3 0.90, config 4 > 3.  Config 2 stays unpartitioned: nothing to gain on three boxes of
    // four, and a capped launch is priced against the whole chip in bench.py's roofline line; MMHIP_PART=96,160 turns it on)
    if (tower(rv, Hv, Iv, c.layers_img, 256) < 1.3 * tower(rt, H, I, c.layers_txt, 256)) return;
    double best = 1e30; int bt = 0;
    for (int t = 32; t <= 224; t += 8) {
        const double ct = tower(rt, H, I, c.layers_txt, t), cv = tower(rv, Hv, Iv, c.layers_img, 256 - t);
        const double m = ct > cv ? ct : cv;
        if (m < best) { best = m; bt = t; }
    }
    if (bt) { e.cur_part[0] = bt; e.cur_part[1] = 256 - bt; }
}

const char* text_last(const mmhip_engine& e) { return e.cfg.layers_txt ? e.ws + e.tact[e.cfg.layers_txt - 1].out : e.ws + e.x0; }

int heads_forward(mmhip_engine& e, float* out_cls, float* logits, float* out_tim, float* feats_out, hipStream_t s) {
    const mmhip_config& c = e.cfg;
    const int H = c.hidden, E = c.proj_dim, C = c.num_labels, T = e.T, B = e.B, Bt = e.Bt, dt = e.dt();
    const int P = e.P(), Hv = e.Hv(), ZW = H + Hv;     // z = [x_t CLS | image feature]: H + Hv wide
    const float* W = e.train;
    const char* xt = text_last(e);
    const int cs = e.cls_compact ? H : T * H;           // row stride of the CLS rows of the last hidden state
    // z = [x_t CLS | fused image feature]; the fp32 copy of the CLS rows in z[:, :H] is also the A operand of the text pooler and of
    // fc_Q (the 16-bit rows would send small_gemm down its scalar-load path: 21 us instead of 11)
    float* z = e.wsp<float>(e.h_z);
    CHECK_HIP(launch_gather_rows_f32(xt, (size_t)cs, z, ZW, Bt, H, dt, s));
    // text pooler (first B posts) and ITC similarity -- HF dual encoder :261-274
    e.itc_done = !(e.skip_itc && logits == nullptr);
    const bool aspect = e.aspect();          // the aspect-att fusion consumes the text pooler's output itself: computed with or without ITC
    if (e.itc_done || aspect)
        CHECK_HIP(launch_small_nt(small(z, ZW, W + e.t_pool_w, H, W + e.t_pool_b, e.wsp<float>(e.h_tpool), H, B, H, H, ACT_TANH), DT_F32, s));
    if (e.itc_done) {
        CHECK_HIP(launch_small_nt(small(e.wsp<float>(e.h_tpool), H, W + e.tproj_w, H, nullptr, e.wsp<float>(e.h_txt_e), E, B, E, H), DT_F32, s));
        CHECK_HIP(launch_small_nt(small(e.wsp<float>(e.h_vpool), Hv, W + e.vproj_w, Hv, nullptr, e.wsp<float>(e.h_img_e), E, B, E, Hv), DT_F32, s));
        ItcArgs it{e.wsp<float>(e.h_txt_e), e.wsp<float>(e.h_img_e), W + e.logit_scale, e.wsp<float>(e.h_txt_n), e.wsp<float>(e.h_img_n),
                   e.wsp<float>(e.h_txt_inv), e.wsp<float>(e.h_img_inv), e.wsp<float>(e.h_logits), B, E};
        CHECK_HIP(launch_itc_fwd(it, s));
    }
    if (c.fusion == MMHIP_FUSION_ATTENTION) {
        CHECK_HIP(launch_small_nt(small(z, ZW, W + e.fq_w, H, W + e.fq_b, e.wsp<float>(e.h_q), H, Bt, H, H), DT_F32, s));
        CHECK_HIP(launch_small_nn(small(e.wsp<float>(e.h_q), H, W + e.fk_w, H, nullptr, e.wsp<float>(e.h_qk), H, Bt, H, H), s));
        FusionAttnArgs fa{e.wsp<float>(e.h_qk), e.ws + e.v_out, e.wsp<float>(e.h_prob), e.wsp<float>(e.h_xbar), Bt, B, P, H, 1.0f / sqrtf((float)H)};
        CHECK_HIP(launch_fusion_attn_fwd(fa, dt, s));
        CHECK_HIP(launch_small_nt(small(e.wsp<float>(e.h_xbar), H, W + e.fv_w, H, W + e.fv_b, z + H, ZW, Bt, H, H), DT_F32, s));
    } else if (aspect) {
        // mm_late.py:115-131 on the two pooler outputs (Bt == B: mmhip_forward refuses ITM rows); writes feats directly -- no linear_fusion
        CHECK_HIP(launch_aspect_fusion_fwd(aspect_fusion(e.wsp<float>(e.h_tpool), e.wsp<float>(e.h_vpool), W + e.asp_w, W + e.asp_b, B, H,
                                                         e.wsp<float>(e.h_feats), e.wsp<float>(e.h_asp_w), e.wsp<float>(e.h_asp_e)), s));
    } else {
        // concat: image CLS row of post bt % B -- two strided copies (original rows, ITM rows)
        CHECK_HIP(launch_gather_rows_f32(e.ws + e.v_out, (size_t)P * Hv, z + H, ZW, B, Hv, dt, s));
        if (Bt > B) CHECK_HIP(launch_gather_rows_f32(e.ws + e.v_out, (size_t)P * Hv, z + (size_t)B * ZW + H, ZW, B, Hv, dt, s));
    }
    float* feats = e.wsp<float>(e.h_feats);
    if (!aspect) CHECK_HIP(launch_small_nt(small(z, ZW, W + e.fus_w, ZW, W + e.fus_b, feats, H, Bt, H, ZW, ACT_RELU), DT_F32, s));
    CHECK_HIP(launch_elementwise(EW_DROPOUT, feats, nullptr, e.wsp<float>(e.h_featd), (size_t)B * H, 0.f,
                                 make_drop(c.p_head, e.seed, STREAM_HEAD, e.train_mode), s));
    CHECK_HIP(launch_small_nt(small(e.wsp<float>(e.h_featd), H, W + e.cls_w, H, W + e.cls_b, e.wsp<float>(e.h_out_cls), C, B, C, H), DT_F32, s));
    if (e.itm) CHECK_HIP(launch_small_nt(small(feats + (size_t)B * H, H, W + e.tim_w, H, W + e.tim_b, e.wsp<float>(e.h_out_tim), 2, B, 2, H), DT_F32, s));
    if (out_cls) CHECK_HIP(hipMemcpyAsync(out_cls, e.ws + e.h_out_cls, (size_t)B * C * 4, hipMemcpyDeviceToDevice, s));
    if (logits && e.itc_done) CHECK_HIP(hipMemcpyAsync(logits, e.ws + e.h_logits, (size_t)B * B * 4, hipMemcpyDeviceToDevice, s));
    if (out_tim && e.itm) CHECK_HIP(hipMemcpyAsync(out_tim, e.ws + e.h_out_tim, (size_t)B * 2 * 4, hipMemcpyDeviceToDevice, s));
    if (feats_out) CHECK_HIP(hipMemcpyAsync(feats_out, feats, (size_t)B * H * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// ------------------------------------------------------------------------------------------------ backward pieces
// ITC similarity backward down to the text pooler's output: logit_scale and both projections' gradients, d t_pool written (not added) to h_dtpool
int itc_backward_to_tpool(mmhip_engine& e, hipStream_t s) {
    const mmhip_config& c = e.cfg;
    const int H = c.hidden, E = c.proj_dim, B = e.B, Hv = e.Hv();
    const float* W = e.train;
    float* Gd = e.grad;
    if (e.bd_itc_global) {
        // gathered form: this rank's rows of d T_n / d I_n collect both cross-entropy directions over all G posts.  Seed: the loss is the SAME
        // global clip_loss on every rank and each rank differentiates it through its own rows only, so the ranks' parameter gradients sum to
        // the single-process gradient; the exchange then averages (1 / world), hence the factor `world` here
        const int G = e.itc_world * B;
        ItcGlobalBwdArgs gb{};
        gb.txt_n = e.wsp<float>(e.h_g_txt); gb.img_n = e.wsp<float>(e.h_g_img); gb.logit_scale = W + e.logit_scale;
        gb.rowlse = e.wsp<float>(e.h_g_rowlse); gb.collse = e.wsp<float>(e.h_g_collse);
        gb.txt_inv = e.wsp<float>(e.h_txt_inv); gb.img_inv = e.wsp<float>(e.h_img_inv);
        gb.d_txt_n = e.wsp<float>(e.h_g_dtn); gb.d_img_n = e.wsp<float>(e.h_g_din);
        gb.dtxt_e = e.wsp<float>(e.h_dtxt_e); gb.dimg_e = e.wsp<float>(e.h_dimg_e); gb.dlogit_scale = Gd + e.logit_scale;
        gb.ws = e.wsp<float>(e.h_g_ws); gb.G = G; gb.E = E; gb.Bl = B; gb.r0 = e.itc_rank * B;
        gb.scale = e.bd_w_itc * (float)e.itc_world / (2.f * (float)G);
        CHECK_HIP(launch_itc_global_bwd(gb, s));
    } else {
        ItcBwdArgs ib{e.bd_logits, e.wsp<float>(e.h_logits), e.wsp<float>(e.h_txt_n), e.wsp<float>(e.h_img_n), e.wsp<float>(e.h_txt_inv),
                      e.wsp<float>(e.h_img_inv), W + e.logit_scale, e.wsp<float>(e.h_dtxt_e), e.wsp<float>(e.h_dimg_e), Gd + e.logit_scale, B, E};
        CHECK_HIP(launch_itc_bwd(ib, s));
    }
    CHECK_HIP(launch_small_tn(small(e.wsp<float>(e.h_dtxt_e), E, e.wsp<float>(e.h_tpool), H, nullptr, Gd + e.tproj_w, H, B, H, 0, 0, 1), DT_F32, E, s));
    CHECK_HIP(launch_small_tn(small(e.wsp<float>(e.h_dimg_e), E, e.wsp<float>(e.h_vpool), Hv, nullptr, Gd + e.vproj_w, Hv, B, Hv, 0, 0, 1), DT_F32, E, s));
    CHECK_HIP(launch_small_nn(small(e.wsp<float>(e.h_dtxt_e), E, W + e.tproj_w, H, nullptr, e.wsp<float>(e.h_dtpool), H, B, H, E), s));
    return 0;
}
// t_pool = tanh(dense(CLS)) backward from h_dtpool: the pooler's gradients, and d CLS added to (accumulate) or written into h_dxcls
int text_pooler_backward(mmhip_engine& e, int accumulate, hipStream_t s) {
    const int H = e.cfg.hidden, B = e.B, ZW = H + e.Hv();
    const float* W = e.train;
    float* Gd = e.grad;
    const float* z = e.wsp<float>(e.h_z);
    CHECK_HIP(launch_elementwise(EW_TANH_BWD, e.wsp<float>(e.h_dtpool), e.wsp<float>(e.h_tpool), e.wsp<float>(e.h_dprepool), (size_t)B * H, 0.f,
                                 make_drop(0.f, 0, 0, false), s));
    CHECK_HIP(launch_small_tn(small(e.wsp<float>(e.h_dprepool), H, z, ZW, nullptr, Gd + e.t_pool_w, H, B, H, 0, 0, 1), DT_F32, H, s));
    CHECK_HIP(launch_bias_grad_f32(e.wsp<float>(e.h_dprepool), B, H, H, Gd + e.t_pool_b, 1, s));
    CHECK_HIP(launch_small_nn(small(e.wsp<float>(e.h_dprepool), H, W + e.t_pool_w, H, nullptr, e.wsp<float>(e.h_dxcls), H, B, H, H, ACT_NONE, accumulate), s));
    return 0;
}
int heads_backward(mmhip_engine& e, hipStream_t s) {
    const mmhip_config& c = e.cfg;
    const int H = c.hidden, E = c.proj_dim, C = c.num_labels, T = e.T, B = e.B, Bt = e.Bt, dt = e.dt();
    const int P = e.P(), Hv = e.Hv(), ZW = H + Hv;     // z = [x_t CLS | image feature]: H + Hv wide
    const float* W = e.train;
    float* Gd = e.grad;
    const float* d_out_cls = e.bd_out_cls ? e.bd_out_cls : e.wsp<float>(e.h_d_out_cls);
    const float* d_logits = e.bd_logits;
    const float* d_out_tim = e.bd_out_tim;
    float* dfeats = e.wsp<float>(e.h_dfeats);
    float* feats = e.wsp<float>(e.h_feats);
    float* z = e.wsp<float>(e.h_z);
    float* dxcls = e.wsp<float>(e.h_dxcls);
    const DropCfg nodrop = make_drop(0.f, 0, 0, false);
    // classifier: out_cls = linear_cls(dropout(feats[:B]))
    CHECK_HIP(launch_small_nn(small(d_out_cls, C, W + e.cls_w, H, nullptr, dfeats, H, B, H, C), s));
    CHECK_HIP(launch_elementwise(EW_DROPOUT, dfeats, nullptr, dfeats, (size_t)B * H, 0.f, make_drop(c.p_head, e.seed, STREAM_HEAD, e.train_mode), s));
    if (e.bd_feats) CHECK_HIP(launch_elementwise(EW_ADD, dfeats, e.bd_feats, dfeats, (size_t)B * H, 1.f, nodrop, s));
    CHECK_HIP(launch_small_tn(small(d_out_cls, C, e.wsp<float>(e.h_featd), H, nullptr, Gd + e.cls_w, H, B, H, 0, 0, 1), DT_F32, C, s));
    CHECK_HIP(launch_bias_grad_f32(d_out_cls, B, C, C, Gd + e.cls_b, 1, s));
    if (e.itm) {
        if (d_out_tim) {
            CHECK_HIP(launch_small_nn(small(d_out_tim, 2, W + e.tim_w, H, nullptr, dfeats + (size_t)B * H, H, B, H, 2), s));
            CHECK_HIP(launch_small_tn(small(d_out_tim, 2, feats + (size_t)B * H, H, nullptr, Gd + e.tim_w, H, B, H, 0, 0, 1), DT_F32, 2, s));
            CHECK_HIP(launch_bias_grad_f32(d_out_tim, B, 2, 2, Gd + e.tim_b, 1, s));
        } else {
            CHECK_HIP(hipMemsetAsync(dfeats + (size_t)B * H, 0, (size_t)B * H * 4, s));
        }
    }
    // every fusion ends here -- gradient of the last hidden state: CLS rows only (compact [Bt, H] when the last layer ran on CLS rows)
    auto scatter_dxcls = [&]() -> int {
        CHECK_HIP(launch_scatter_cls_rows(dxcls, e.ws + e.g_dx, Bt, e.cls_compact ? 1 : T, H, dt, s, e.gscale()));
        return 0;
    };
    if (e.aspect()) {
        // feats = relu(sum_j w_j V_j) over the stacked pooler outputs: ITC's gradient of t_pool first (a plain write), the fusion's added to it by the
        // rows' one writer; then the text pooler's backward, which OPENS dxcls here (nothing else reaches the CLS rows under this fusion)
        const bool itc = d_logits || e.bd_itc_global;
        if (itc) CHECK_RC(itc_backward_to_tpool(e, s));
        AspectFusionArgs ab = aspect_fusion(e.wsp<float>(e.h_tpool), e.wsp<float>(e.h_vpool), W + e.asp_w, W + e.asp_b, B, H, feats,
                                            e.wsp<float>(e.h_asp_w), e.wsp<float>(e.h_asp_e));
        ab.d_feats = dfeats; ab.d_tpool = e.wsp<float>(e.h_dtpool); ab.da = Gd + e.asp_w; ab.db = Gd + e.asp_b;
        ab.partial = e.wsp<float>(e.h_asp_partial); ab.accumulate = itc; ab.accumulate_dw = 1;
        CHECK_HIP(launch_aspect_fusion_bwd(ab, s));
        CHECK_RC(text_pooler_backward(e, 0, s));
        return scatter_dxcls();
    }
    // feats = relu(linear_fusion(z))
    float* dpre = e.wsp<float>(e.h_dpre);
    CHECK_HIP(launch_elementwise(EW_RELU_BWD, dfeats, feats, dpre, (size_t)Bt * H, 0.f, nodrop, s));
    CHECK_HIP(launch_small_tn(small(dpre, H, z, ZW, nullptr, Gd + e.fus_w, ZW, Bt, ZW, 0, 0, 1), DT_F32, H, s));
    CHECK_HIP(launch_bias_grad_f32(dpre, Bt, H, H, Gd + e.fus_b, 1, s));
    float* dz = e.wsp<float>(e.h_dz);
    CHECK_HIP(launch_small_nn(small(dpre, H, W + e.fus_w, ZW, nullptr, dz, ZW, Bt, ZW, H), s));
    // d x_t[:,0] starts as dz[:, :H]
    CHECK_HIP(hipMemcpy2DAsync(dxcls, (size_t)H * 4, dz, (size_t)ZW * 4, (size_t)H * 4, Bt, hipMemcpyDeviceToDevice, s));
    if (c.fusion == MMHIP_FUSION_ATTENTION) {
        const float* dctx = dz + H;      // ld ZW
        float* q = e.wsp<float>(e.h_q);
        CHECK_HIP(launch_small_tn(small(dctx, ZW, e.wsp<float>(e.h_xbar), H, nullptr, Gd + e.fv_w, H, Bt, H, 0, 0, 1), DT_F32, H, s));
        CHECK_HIP(launch_bias_grad_f32(dctx, Bt, H, ZW, Gd + e.fv_b, 1, s));
        CHECK_HIP(launch_small_nn(small(dctx, ZW, W + e.fv_w, H, nullptr, e.wsp<float>(e.h_dxbar), H, Bt, H, H), s));
        FusionAttnBwdArgs fb{e.wsp<float>(e.h_dxbar), e.wsp<float>(e.h_prob), e.ws + e.v_out, e.wsp<float>(e.h_dqk), Bt, B, P, H, 1.0f / sqrtf((float)H)};
        CHECK_HIP(launch_fusion_attn_bwd(fb, dt, s));
        // qk = q . W_K  ->  dW_K[o][i] = sum q[:,o] dqk[:,i];  dq = dqk . W_K^T ;  fc_K.bias gets an exactly-zero gradient
        CHECK_HIP(launch_small_tn(small(q, H, e.wsp<float>(e.h_dqk), H, nullptr, Gd + e.fk_w, H, Bt, H, 0, 0, 1), DT_F32, H, s));
        CHECK_HIP(launch_small_nt(small(e.wsp<float>(e.h_dqk), H, W + e.fk_w, H, nullptr, e.wsp<float>(e.h_dq), H, Bt, H, H), DT_F32, s));
        CHECK_HIP(launch_small_tn(small(e.wsp<float>(e.h_dq), H, z, ZW, nullptr, Gd + e.fq_w, H, Bt, H, 0, 0, 1), DT_F32, H, s));
        CHECK_HIP(launch_bias_grad_f32(e.wsp<float>(e.h_dq), Bt, H, H, Gd + e.fq_b, 1, s));
        CHECK_HIP(launch_small_nn(small(e.wsp<float>(e.h_dq), H, W + e.fq_w, H, nullptr, dxcls, H, Bt, H, H, ACT_NONE, 1), s));
    }
    if (d_logits || e.bd_itc_global) {
        CHECK_RC(itc_backward_to_tpool(e, s));
        CHECK_RC(text_pooler_backward(e, 1, s));
    }
    return scatter_dxcls();
}

// ---- one-tower handles: the fused CLS classifier head (heads.hip), one launch per direction.  txt_head_args / img_head_args: where each kind's CLS rows are
ClsHeadArgs txt_head_args(const mmhip_engine& e) {
    const mmhip_config& c = e.cfg;
    // parity mode keeps the fp32 form of the last hidden state beside its plane pair: the head reads that
    return cls_head(text_last(e), e.cls_compact ? (size_t)c.hidden : (size_t)e.T * c.hidden, e.dt(), e.train + e.lin_w, e.B, c.num_labels, c.hidden,
                    make_drop(c.p_head, e.seed, STREAM_HEAD, e.train_mode));
}
// logits of the head over the rows `a` names (and, with labels, loss / correct count / d logits kept in the handle for the backward)
int cls_head_forward(mmhip_engine& e, ClsHeadArgs a, const int64_t* onehot, const float* class_w, float* logits, float* loss, int* n_correct, hipStream_t s) {
    a.bias = e.train + e.lin_b; a.logits = e.wsp<float>(e.h_out_cls);
    if (onehot) {
        a.onehot = onehot; a.class_w = class_w; a.loss = e.wsp<float>(e.h_loss); a.n_correct = n_correct; a.d_logits_out = e.wsp<float>(e.h_d_out_cls);
    }
    CHECK_HIP(launch_cls_head_fwd(a, s));
    if (logits) CHECK_HIP(hipMemcpyAsync(logits, a.logits, (size_t)e.B * e.cfg.num_labels * 4, hipMemcpyDeviceToDevice, s));
    if (onehot && loss) CHECK_HIP(hipMemcpyAsync(loss, a.loss, 4, hipMemcpyDeviceToDevice, s));
    if (onehot) e.bd_out_cls = a.d_logits_out;
    return 0;
}
int txt_head_backward(mmhip_engine& e, hipStream_t s) {
    const int H = e.cfg.hidden;
    ClsHeadArgs a = txt_head_args(e);
    a.d_logits = e.bd_out_cls; a.dW = e.grad + e.lin_w; a.db = e.grad + e.lin_b; a.accumulate = 1;
    if (e.cls_compact) {          // straight into the compact CLS-row gradient the last layer's backward consumes
        a.dx = e.ws + e.g_dx; a.dx_stride = H; a.dx_dtype = e.dt(); a.dx_scale = e.gscale();
        CHECK_HIP(launch_cls_head_bwd(a, s));
        return 0;
    }
    // MMHIP_CLS_ONLY=0 (or no layer): fp32 rows, spread into the otherwise-zero full gradient tensor
    a.dx = e.wsp<float>(e.h_dxcls); a.dx_stride = H; a.dx_dtype = DT_F32; a.dx_scale = 1.f;
    CHECK_HIP(launch_cls_head_bwd(a, s));
    CHECK_HIP(launch_scatter_cls_rows(e.wsp<float>(e.h_dxcls), e.ws + e.g_dx, e.Bt, e.T, H, e.dt(), s, e.gscale()));
    return 0;
}

// ---- the weight-gradient tail of a layer's backward, the same under both towers.  The temporaries the weight-gradient GEMMs read are double-buffered
// per layer parity (`set`), so the side stream may still be consuming layer l's set while the caller's stream runs layer l - 1 on the other one.
// join_set: `s` waits for the side work that last read `set` (layer l + 2's; at the end of a backward: every gradient final in the caller's order)
int join_set(mmhip_engine& e, int set, hipStream_t s) {
    if (e.tn_pending[set]) {
        CHECK_HIP(hipStreamWaitEvent(s, e.ev_tn[set], 0));
        e.tn_pending[set] = false;
    }
    return 0;
}
// everything the layer's parameter gradients read has been enqueued on `s`: ps = the stream they go to -- the side stream, made to wait for this
// point of `s`, or `s` itself with the side stream off
int fork_param_grads(mmhip_engine& e, int set, hipStream_t s, hipStream_t& ps) {
    ps = s;
    if (use_side(e)) {
        CHECK_HIP(hipEventRecord(e.ev_ready[set], s));
        CHECK_HIP(hipStreamWaitEvent(e.side, e.ev_ready[set], 0));
        ps = e.side;
    }
    return 0;
}
// parameter gradients of the layer on ps, off the dX chain: the second stage of the two LayerNorm reductions, then all four weight gradients AND
// their bias gradients (column sums of the dY operand, from the same tiles) in one grouped launch, no split-K, plain stores
int layer_param_grads(mmhip_engine& e, int set, hipStream_t ps, const LNBwdArgs& b2, const LNBwdArgs& b1, GemmTNProblem (&pr)[4]) {
    CHECK_HIP(launch_layernorm_bwd_reduce(b2, ps));
    CHECK_HIP(launch_layernorm_bwd_reduce(b1, ps));
    if (e.px) for (auto& q : pr) tn_pair(q, e.bwd_np);
    const X3Scratch x = x3_scratch(e, ps);
    CHECK_HIP(launch_gemm_tn(pr, 4, 0, e.dt(), 0, ps, 1.0f / e.gscale(), x.ws, x.bytes));
    if (e.side && ps == e.side) {
        CHECK_HIP(hipEventRecord(e.ev_tn[set], e.side));
        e.tn_pending[set] = true;
    }
    return 0;
}

// one text layer; on entry g_dx holds the gradient of the layer's output, on exit of its input
int text_layer_backward(mmhip_engine& e, int l, hipStream_t s) {
    const mmhip_config& c = e.cfg;
    const int H = c.hidden, I = c.inter, T = e.T, Bt = e.Bt, Mt = Bt * T, dt = e.dt();
    const float* W = e.train;
    float* Gd = e.grad;
    const LayerOff& o = e.txt[l];
    const LayerW16& w = e.txt_w16[l];
    const TextAct& a = e.tact[l];
    const bool px = e.px;
    const int np = e.bwd_np;          // parity mode: MFMA products per k slice of the backward's GEMMs (mmhip_set_backward_products)
    const bool hi1 = px && np == 1;   // one product everywhere downstream: the lo planes of du / d ctx / d qkv / the dropped LayerNorm gradients are never read -- not written
    const char* x_in = px ? (l ? e.ws + e.tact[l - 1].outp : e.ws + e.x0p) : (l ? e.ws + e.tact[l - 1].out : e.ws + e.x0);      // as the dWqkv product reads it
    const bool tr = e.train_mode;
    // temporaries that the weight-gradient GEMMs read are double-buffered per layer parity so that the side stream may
    // still be consuming layer l's set while the main stream runs layer l-1 on the other one
    const int set = l & 1;
    // last layer in CLS-only mode: its gradient arrives as compact [Bt, H] rows; everything up to d ctx runs on Bt rows
    const bool compact = e.cls_compact && l == c.layers_txt - 1;
    const int Mr = compact ? Bt : Mt, rs = compact ? T * H : H, rmul = compact ? T : 1;
    char *dx = e.ws + e.g_dx, *dx2 = e.ws + e.g_dx2, *dctx = e.ws + e.g_dctx;
    char *dpre2 = e.ws + e.g_set[set][0], *ddrop2 = e.ws + e.g_set[set][1], *du = e.ws + e.g_set[set][2];
    char *dpre1 = e.ws + e.g_set[set][3], *ddrop1 = e.ws + e.g_set[set][4], *dqkv = e.ws + e.g_set[set][5];
    CHECK_RC(join_set(e, set, s));           // the set was last read by layer l+2's side work
    // ---- x' = LN2(pre2), pre2 = drop(fc2(h)) + a1.  LN backward also emits the dropout-backward copy and the bias
    // gradient of the Linear that fed the LN
    const DropCfg d_ffn = make_drop(c.p_hidden, e.seed, stream_ffn_out(l), tr);
    // (the second stage of its dgamma / dbeta reduction is not on the dX chain: it runs with the layer's dW on the side stream)
    LNBwdArgs b2{dx, e.ws + a.pre2, W + o.ln2_w, e.wsp<float>(a.mean2), e.wsp<float>(a.rstd2), dpre2, nullptr, Gd + o.ln2_w, Gd + o.ln2_b, Mr, H,
                 e.wsp<float>(e.g_lnp[set][0]), 1.0f / e.gscale(), d_ffn.thresh16 ? ddrop2 : nullptr, nullptr, d_ffn, rmul, 1};
    ln_bwd_pair(b2, px, ddrop2, hi1);      // parity mode: the GEMMs' operand (dropped or not) as a plane pair in the ddrop buffer
    CHECK_HIP(launch_layernorm_bwd(b2, dt, s));
    const char* df = (px || d_ffn.thresh16) ? ddrop2 : dpre2;
    // du = (df . W2) * gelu'(u);  d_a1 = du . W1 + dpre2
    { G g(df, H, e.ws + w.fc2T, H, du, I, Mr, I, H); g.mul_gelu_grad(e.ws + a.u, I).px_in(px, np).px_out(px, hi1); CHECK_RC(run_gemm(e, g, s)); }
    // the two long-K activation-gradient GEMMs of the layer (768 wide): one role-specialised 256x96 tile per CU when M gives
    // exactly <= 256 of them -- in isolation 7 % faster than the 192 tiles of 256x128, in the step -0.05 ms (same-box A/B; the
    // same tile in the FORWARD costs +0.3 ms: it leaves no CU to the image tower).  The non-compact
    // d ctx GEMM below (K = H) keeps the launcher's own choice.
    const int nt = (Mr >= 4096 && Mr <= 8192 && H % 96 == 0) ? 12 : 0;
    { G g(du, I, e.ws + w.fc1T, I, dx2, H, Mr, H, I); g.residual(dpre2, H).px_in(px, np); g.tile(nt); CHECK_RC(run_gemm(e, g, s)); }
    // ---- a1 = LN1(pre1), pre1 = drop(ao(ctx)) + x_in        (dx2 = d_a1)
    const DropCfg d_ao = make_drop(c.p_hidden, e.seed, stream_attn_out(l), tr);
    LNBwdArgs b1{dx2, e.ws + a.pre1, W + o.ln1_w, e.wsp<float>(a.mean1), e.wsp<float>(a.rstd1), dpre1, nullptr, Gd + o.ln1_w, Gd + o.ln1_b, Mr, H,
                 e.wsp<float>(e.g_lnp[set][1]), 1.0f / e.gscale(), d_ao.thresh16 ? ddrop1 : nullptr, nullptr, d_ao, rmul, 1};
    ln_bwd_pair(b1, px, ddrop1, hi1);
    CHECK_HIP(launch_layernorm_bwd(b1, dt, s));
    const char* dout = (px || d_ao.thresh16) ? ddrop1 : dpre1;
    if (compact) {
        // d ctx for the CLS rows only, spread into an otherwise-zero full tensor for the attention backward (parity mode: pair rows of 2 H 16-bit
        // elements are moved as the H 4-byte words they occupy; an all-zero pair is zero)
        { G g(dout, H, e.ws + w.aoT, H, dx2, H, Mr, H, H); g.px_in(px, np).px_out(px, hi1); CHECK_RC(run_gemm(e, g, s)); }
        CHECK_HIP(hipMemsetAsync(dctx, 0, (size_t)Mt * H * e.esz(), s));
        CHECK_HIP(launch_scatter_rows16(dx2, dctx, Bt, (size_t)T * H, H, 0, dt, s));
        CHECK_HIP(hipMemsetAsync(dqkv, 0, (size_t)Mt * 3 * H * e.esz(), s));      // dQ of the skipped query tiles is zero
    } else {
        G g(dout, H, e.ws + w.aoT, H, dctx, H, Mt, H, H);
        g.px_in(px, np).px_out(px, hi1);
        CHECK_RC(run_gemm(e, g, s));
    }
    AttnBwdArgs ab = attn_bwd_args(e.ws + a.qkv, e.wsp<float>(e.maskbias), e.ws + a.ctx, dctx, e.wsp<float>(a.lse), dqkv, Bt, T, c.heads, H,
                                   make_drop(c.p_attn, e.seed, stream_attn(l), tr));
    attn_pair(ab, px, np);
    ab.q_tiles = compact ? 1 : 0;
    CHECK_HIP(launch_attn_bwd(ab, dt, s));
    // ---- parameter gradients of the layer: off the critical path -> side stream, forked BEFORE the last dX GEMM (which they do not read)
    hipStream_t ps;
    CHECK_RC(fork_param_grads(e, set, s, ps));
    if (compact) {
        // dx_in = dqkv . Wqkv, plus d pre1 on the CLS rows (the residual branch of the CLS rows)
        { G g(dqkv, 3 * H, e.ws + w.qkvT, 3 * H, dx, H, Mt, H, 3 * H); g.px_in(px, np); CHECK_RC(run_gemm(e, g, s)); }
        CHECK_HIP(launch_scatter_rows16(dpre1, dx, Bt, (size_t)T * H, H, 1, dt, s));
    } else {
        G g(dqkv, 3 * H, e.ws + w.qkvT, 3 * H, dx, H, Mt, H, 3 * H);
        g.residual(dpre1, H).px_in(px, np);
        g.tile(nt);
        CHECK_RC(run_gemm(e, g, s));
    }
    GemmTNProblem pr[4] = {
        {df, e.ws + a.h, Gd + o.fc2_w, Mr, H, I, H, I, I, 0, Gd + o.fc2_b},                                  // dW2[H,I]   = df^T h
        {du, e.ws + (px ? a.a1p : a.a1), Gd + o.fc1_w, Mr, I, H, I, H, H, 0, Gd + o.fc1_b},                  // dW1[I,H]   = du^T a1 (its plane pair)
        {dqkv, x_in, Gd + o.qkv_w, Mt, 3 * H, H, 3 * H, H, H, 0, Gd + o.qkv_b},                              // dWqkv[3H,H] = dqkv^T x_in
        {dout, e.ws + a.ctx, Gd + o.ao_w, Mr, H, H, H, rs, H, 0, Gd + o.ao_b}};                              // dWo[H,H]   = dout^T ctx (CLS rows: stride T*H)
    return layer_param_grads(e, set, ps, b2, b1, pr);
}

// join the side stream: after this, every gradient is final in the caller's stream order
int backward_finish(mmhip_engine& e, hipStream_t s) {
    for (int set = 0; set < 2; ++set) CHECK_RC(join_set(e, set, s));
    return 0;
}

// device words of the overflow guard: [0] counter of non-finite gradient sightings, [1] "this step is void" flag raised by the backward and
// honoured by the AdamW kernels.  Per handle (mmhip_set_guard; round 4: two models in one process no longer share a flag); the process-wide
// pair of mmhip_set_step_guard / mmhip_set_nonfinite_counter serves the handle-less AdamW entry points and handles without a guard of their own.
static unsigned* g_nonfinite = nullptr;
static unsigned* g_skip = nullptr;
inline unsigned* guard_counter(const mmhip_engine& e) { return e.guard ? e.guard : g_nonfinite; }
inline unsigned* guard_flag(const mmhip_engine& e) { return e.guard ? e.guard + 1 : g_skip; }

int embed_backward(mmhip_engine& e, hipStream_t s) {
    const mmhip_config& c = e.cfg;
    const float* W = e.train;
    float* Gd = e.grad;
    EmbedBwdArgs b{};
    b.dx = e.ws + e.g_dx; b.xhat = e.ws + e.xhat_emb; b.rstd = e.wsp<float>(e.rstd_emb); b.gamma = W + e.t_eln_w;
    b.ids = e.wsp<int64_t>(e.ids_all); b.pos_ids = e.wsp<int>(e.pos_ids);
    b.dword = Gd + e.t_word; b.dpos = Gd + e.t_pos; b.dtype = Gd + e.t_type; b.dgamma = Gd + e.t_eln_w; b.dbeta = Gd + e.t_eln_b;
    b.posts = e.Bt; b.T = e.T; b.H = c.hidden; b.pad_id = c.pad_id;
    b.pos_pad_id = c.txt_kind == MMHIP_TXT_XLMR ? c.pad_id : -1;     // nn.Embedding(padding_idx=...) rows get no gradient
    b.drop = make_drop(c.p_hidden, e.seed, STREAM_EMBED, e.train_mode);
    b.partial = e.wsp<float>(e.g_partial);
    b.alpha = 1.0f / e.gscale();
    b.row_state = e.word_row_state;
    if (e.has_tt) { b.type_ids = e.wsp<int64_t>(e.tt_all); b.type_rows = 2; }      // BERT's two-row table: both rows take their tokens' gradient
    if (deterministic()) { b.det_rows = e.wsp<float>(e.g_det_rows); b.max_pos = c.max_pos; }
    b.status = guard_flag(e) ? guard_counter(e) : nullptr;
    CHECK_HIP(launch_embed_bwd(b, e.dt(), s));
    return 0;
}

// parity mode: operands as plane pairs or split per call (MMHIP_X3_PAIRS), MFMA products per k slice of the backward (MMHIP_X3_BWD); read at create
void read_x3_env(mmhip_engine& e) {
    if (e.cfg.dtype != MMHIP_BF16X3) return;
    e.px = env_int("MMHIP_X3_PAIRS", 1) != 0;
    const int n = env_int("MMHIP_X3_BWD", 3);
    e.bwd_np = n >= 1 && n <= 3 ? n : 3;
}

// ------------------------------------------------------------------------------------------------ image-only handle: forward and backward pieces
// clears the pad rows (mmhip_engine::i_pad_B) of every operand of a weight-gradient product for B posts
int img_zero_pads(mmhip_engine& e, int B, hipStream_t s) {
    const size_t H = e.Hv(), I = e.Iv(), P = e.P(), Z = e.esz();
    const size_t Mv = B * P, Mvp = mmhip_engine::pad64(Mv), Mp = (size_t)B * (P - 1), Mpp = mmhip_engine::pad64(Mp);
    auto clear = [&](size_t off, size_t rows, size_t rows_padded, size_t width) -> int {
        if (rows_padded > rows) CHECK_HIP(hipMemsetAsync(e.ws + off + rows * width * Z, 0, (rows_padded - rows) * width * Z, s));
        return 0;
    };
    for (const ImgAct& a : e.iact) {
        CHECK_RC(clear(a.ln1, Mv, Mvp, H)); CHECK_RC(clear(a.ln2, Mv, Mvp, H)); CHECK_RC(clear(a.ctx, Mv, Mvp, H)); CHECK_RC(clear(a.h, Mv, Mvp, I));
    }
    for (int i = 0; i < 3; ++i) {
        CHECK_RC(clear(e.i_dxs[i], Mv, Mvp, H));
        if (e.px) CHECK_RC(clear(e.i_dxs_p[i], Mv, Mvp, H));
    }
    for (int i = 0; i < 2; ++i) {
        CHECK_RC(clear(e.i_set[i][0], Mv, Mvp, I)); CHECK_RC(clear(e.i_set[i][1], Mv, Mvp, 3 * H)); CHECK_RC(clear(e.i_set[i][2], Mv, Mvp, H));
        if (e.px) CHECK_RC(clear(e.i_set[i][3], Mv, Mvp, H));
    }
    CHECK_RC(clear(e.v_patches, Mp, Mpp, e.Kpp()));
    CHECK_RC(clear(e.i_dpe, Mp, Mpp, H));
    e.i_pad_B = B;
    return 0;
}

// classifier(layernorm(x)[:, 0, :]): the B CLS rows gathered, the final LayerNorm on them alone (no other row of it is consumed), the fused head, p = 0
ClsHeadArgs img_head_args(const mmhip_engine& e) {
    return cls_head(e.ws + e.i_clsln, (size_t)e.Hv(), e.dt(), e.train + e.lin_w, e.B, e.cfg.num_labels, e.Hv(), make_drop(0.f, 0, STREAM_HEAD, false));
}
int img_head_forward(mmhip_engine& e, const int64_t* onehot, const float* class_w, float* logits, float* loss, int* n_correct, hipStream_t s) {
    const int H = e.Hv(), B = e.B, P = e.P();
    const size_t rb = (size_t)H * e.esz();
    CHECK_HIP(hipMemcpy2DAsync(e.ws + e.i_cls, rb, e.ws + e.i_xfin, (size_t)P * rb, rb, B, hipMemcpyDeviceToDevice, s));
    LNArgs n{e.ws + e.i_cls, e.ws + e.i_clsln, e.train + e.v_ln_w, e.train + e.v_ln_b, e.wsp<float>(e.i_mean), e.wsp<float>(e.i_rstd), B, H, H, H, e.cfg.ln_eps_img};
    CHECK_HIP(launch_layernorm_fwd(n, e.dt(), s));
    return cls_head_forward(e, img_head_args(e), onehot, class_w, logits, loss, n_correct, s);
}
// stage 0: head, final LayerNorm on the B rows, and the gradient of the last stream: zero but for the CLS rows
int img_head_backward(mmhip_engine& e, hipStream_t s) {
    const int H = e.Hv(), B = e.B, P = e.P(), L = e.cfg.layers_img, dt = e.dt();
    const bool px = e.px, hi1 = px && e.bwd_np == 1;
    ClsHeadArgs a = img_head_args(e);
    a.d_logits = e.bd_out_cls; a.dW = e.grad + e.lin_w; a.db = e.grad + e.lin_b; a.accumulate = 1;
    a.dx = e.ws + e.i_dcls; a.dx_stride = H; a.dx_dtype = dt; a.dx_scale = e.gscale();
    CHECK_HIP(launch_cls_head_bwd(a, s));
    LNBwdArgs b{e.ws + e.i_dcls, e.ws + e.i_cls, e.train + e.v_ln_w, e.wsp<float>(e.i_mean), e.wsp<float>(e.i_rstd), e.ws + e.i_dclsx, nullptr,
                e.grad + e.v_ln_w, e.grad + e.v_ln_b, B, H, e.wsp<float>(e.g_partial), 1.0f / e.gscale(), nullptr, nullptr, make_drop(0.f, 0, 0, false), 1, 0};
    ln_bwd_pair(b, px, e.ws + e.i_dclsx_p, hi1);
    CHECK_HIP(launch_layernorm_bwd(b, dt, s));
    const size_t bytes = (size_t)B * P * H * e.esz();
    CHECK_HIP(hipMemsetAsync(e.ws + e.i_dxs[L % 3], 0, bytes, s));
    CHECK_HIP(launch_scatter_rows16(e.ws + e.i_dclsx, e.ws + e.i_dxs[L % 3], B, (size_t)P * H, H, 0, dt, s));
    if (px) {          // the pair the layer's GEMMs read: rows of 2 H bf16 moved as the H 4-byte words they occupy; an all-zero pair is zero
        CHECK_HIP(hipMemsetAsync(e.ws + e.i_dxs_p[L % 3], 0, bytes, s));
        CHECK_HIP(launch_scatter_rows16(e.ws + e.i_dclsx_p, e.ws + e.i_dxs_p[L % 3], B, (size_t)P * H, H, 0, DT_F32, s));
    }
    return 0;
}

// One pre-LN image layer: x_mid = x_in + Wo ctx(LN1(x_in)),  x_out = x_mid + W2 gelu(W1 LN2(x_mid)).  On entry the gradient of x_out is in the
// stream-gradient buffer (l + 1) % 3, on exit that of x_in in l % 3 (three of them: the layer's weight-gradient launch on the side stream still reads
// the first while the layer below writes its own).  LNBwdArgs::dres adds the residual branch's gradient inside the LayerNorm backward.
int image_layer_backward(mmhip_engine& e, int l, hipStream_t s) {
    const int H = e.Hv(), I = e.Iv(), B = e.B, P = e.P(), Mv = B * P, dt = e.dt();
    const float* W = e.train;
    float* Gd = e.grad;
    const LayerOff& o = e.vit[l];
    const LayerW16& w = e.vit_w16[l];
    const ImgAct& a = e.iact[l];
    const bool px = e.px;
    const int np = e.bwd_np;
    const bool hi1 = px && np == 1;          // every reader takes one product: lo planes not written (d ctx excepted: the attention backward keeps three)
    const int set = l & 1;
    const int di = (l + 1) % 3, dn = l % 3;
    char *dx = e.ws + e.i_dxs[di], *dxg = px ? e.ws + e.i_dxs_p[di] : dx;                      // fp32 / 16-bit form, and as the GEMMs read it
    char *dxo = e.ws + e.i_dxs[dn], *dxo_p = e.ws + e.i_dxs_p[dn];
    char *du = e.ws + e.i_set[set][0], *dqkv = e.ws + e.i_set[set][1], *dxmid = e.ws + e.i_set[set][2];
    char *dxmid_g = px ? e.ws + e.i_set[set][3] : dxmid;
    char *dln = e.ws + e.i_dln, *dctx = e.ws + e.i_dctx;
    CHECK_RC(join_set(e, set, s));           // the set was last read by layer l+2's side work
    const DropCfg nodrop = make_drop(0.f, 0, 0, false);
    // du = (dx . W2) * gelu'(u);  d ln2 = du . W1;  dx_mid = LNbwd(d ln2; x_mid) + dx
    CHECK_RC(run_gemm(e, G(dxg, H, e.ws + w.fc2T, H, du, I, Mv, I, H).mul_gelu_grad(e.ws + a.u, I).px_in(px, np).px_out(px, hi1), s));
    CHECK_RC(run_gemm(e, G(du, I, e.ws + w.fc1T, I, dln, H, Mv, H, I).px_in(px, np), s));
    LNBwdArgs b2{dln, e.ws + a.x_mid, W + o.ln2_w, e.wsp<float>(a.mean2), e.wsp<float>(a.rstd2), dxmid, dx, Gd + o.ln2_w, Gd + o.ln2_b, Mv, H,
                 e.wsp<float>(e.g_lnp[set][0]), 1.0f / e.gscale(), nullptr, nullptr, nodrop, 1, 1};
    ln_bwd_pair(b2, px, dxmid_g, hi1);
    CHECK_HIP(launch_layernorm_bwd(b2, dt, s));
    // d ctx = dx_mid . Wo;  attention backward (129 .. 288 tokens: three products at every policy);  d ln1 = dqkv . Wqkv;  dx_in = LNbwd(d ln1; x_in) + dx_mid
    CHECK_RC(run_gemm(e, G(dxmid_g, H, e.ws + w.aoT, H, dctx, H, Mv, H, H).px_in(px, np).px_out(px), s));
    AttnBwdArgs ab = attn_bwd_args(e.ws + a.qkv, nullptr, e.ws + a.ctx, dctx, e.wsp<float>(a.lse), dqkv, B, P, e.heads_v(), H);
    attn_pair(ab, px, np == 1 ? 3 : np);
    CHECK_HIP(launch_attn_bwd_long(ab, dt, s));
    CHECK_RC(run_gemm(e, G(dqkv, 3 * H, e.ws + w.qkvT, 3 * H, dln, H, Mv, H, 3 * H).px_in(px, np), s));
    LNBwdArgs b1{dln, e.ws + a.x_in, W + o.ln1_w, e.wsp<float>(a.mean1), e.wsp<float>(a.rstd1), dxo, dxmid, Gd + o.ln1_w, Gd + o.ln1_b, Mv, H,
                 e.wsp<float>(e.g_lnp[set][1]), 1.0f / e.gscale(), nullptr, nullptr, nodrop, 1, 1};
    ln_bwd_pair(b1, px, dxo_p, hi1);
    CHECK_HIP(launch_layernorm_bwd(b1, dt, s));
    // ---- parameter gradients of the layer, off the dX chain -> side stream, forked once the whole chain is enqueued
    hipStream_t ps;
    CHECK_RC(fork_param_grads(e, set, s, ps));
    const int Mr = (int)mmhip_engine::pad64((size_t)Mv);          // reduction length with the zero pad rows (i_pad_B)
    GemmTNProblem pr[4] = {
        {dxg, e.ws + a.h, Gd + o.fc2_w, Mr, H, I, H, I, I, 0, Gd + o.fc2_b},                   // dW2[H,I]    = dx^T h
        {du, e.ws + a.ln2, Gd + o.fc1_w, Mr, I, H, I, H, H, 0, Gd + o.fc1_b},                  // dW1[I,H]    = du^T ln2
        {dqkv, e.ws + a.ln1, Gd + o.qkv_w, Mr, 3 * H, H, 3 * H, H, H, 0, Gd + o.qkv_b},        // dWqkv[3H,H] = dqkv^T ln1
        {dxmid_g, e.ws + a.ctx, Gd + o.ao_w, Mr, H, H, H, H, H, 0, Gd + o.ao_b}};              // dWo[H,H]    = dx_mid^T ctx
    return layer_param_grads(e, set, ps, b2, b1, pr);
}

// stage L + 1: d position_embeddings, d cls_token and the compact patch-row gradient in one launch; the patch weight's gradient with its bias
// gradient as one more weight-gradient problem against the forward's patchified pixels (still intact in v_patches)
int img_embed_backward(mmhip_engine& e, hipStream_t s) {
    const int H = e.Hv(), B = e.B, P = e.P(), Kpp = e.Kpp(), dt = e.dt();
    const bool px = e.px;
    VitEmbedBwdArgs v{};
    v.dx = e.ws + e.i_dxs[0]; v.dpos = e.grad + e.v_pos; v.dcls = e.grad + e.v_cls; v.dpe = e.ws + e.i_dpe;
    v.B = B; v.P = P; v.H = H; v.alpha = 1.0f / e.gscale();
    v.partial = partial_floats_vit_embed(B, P, H) ? e.wsp<float>(e.i_epartial) : nullptr;
    if (px) { v.pair = 1; v.pair_hi_only = e.bwd_np == 1; v.ld_pair = 2 * H; v.lo_pair = H; }
    CHECK_HIP(launch_vit_embed_bwd(v, dt, s));
    GemmTNProblem pr{e.ws + e.i_dpe, e.ws + e.v_patches, e.grad + e.v_patch_w, (int)mmhip_engine::pad64((size_t)B * (P - 1)), H, Kpp, H, Kpp, Kpp, 0,
                     e.grad + e.v_patch_b};          // (zero pad rows: i_pad_B)
    if (px) tn_pair(pr, e.bwd_np);
    const X3Scratch x = x3_scratch(e, s);
    CHECK_HIP(launch_gemm_tn(&pr, 1, 0, dt, 0, s, 1.0f / e.gscale(), x.ws, x.bytes));
    return 0;
}

int img_refresh(mmhip_engine& e, hipStream_t s) {
    for (int l = 0; l < e.cfg.layers_img; ++l) CHECK_RC(refresh_layer(e, e.train, e.vit[l], e.vit_w16[l], true, s, e.Hv(), e.Iv()));
    return refresh_patch(e, e.train, s);
}

}  // namespace

// ================================================================================================ C ABI
extern "C" {

const char* mmhip_version(void) { return "mmhip 0.1 (gfx950)"; }

int mmhip_create(const mmhip_config* cfg, mmhip_handle* out) {
    if (!cfg || !out) return MMHIP_E_INVALID;
    const mmhip_config& c = *cfg;
    if (c.hidden <= 0 || c.hidden % 64 || c.hidden > 1024 || c.heads * 64 != c.hidden || c.inter % 128 || c.hidden % 128) return MMHIP_E_INVALID;
    {   // image tower: ViT (HF ViTModel) or CLIP vision (HF CLIPVisionModel), its own width allowed (CLIP-ViT-L/14: 1024 / 16 / 4096)
        const int hv = c.hidden_img > 0 ? c.hidden_img : c.hidden, iv = c.inter_img > 0 ? c.inter_img : c.inter, nh = c.heads_img > 0 ? c.heads_img : c.heads;
        if (c.img_kind != MMHIP_IMG_VIT && c.img_kind != MMHIP_IMG_CLIP && c.img_kind != MMHIP_IMG_BEIT) return MMHIP_E_INVALID;
        if (hv % 128 || hv > 1024 || nh * 64 != hv || iv % 128 || c.patch < 2 || c.image % c.patch) return MMHIP_E_INVALID;
        if (c.fusion == MMHIP_FUSION_ATTENTION && hv != c.hidden) return MMHIP_E_INVALID;       // fc_K / fc_V are hidden x hidden (mm_late.py:74-75)
        if (c.fusion == MMHIP_FUSION_ASPECT && hv != c.hidden) return MMHIP_E_INVALID;          // the two pooler outputs are stacked into one matrix (mm_late.py:120)
        // attention keeps the K / V of a head in LDS: 608 keys of 64 x 16 bit fill the 160 KB of a CU (336 / 14 -> 577 tokens);
        // the fp32 parity-mode attention holds 4-byte K / V: 288 keys
        const int P = (c.image / c.patch) * (c.image / c.patch) + 1;
        if (P > 608) return MMHIP_E_INVALID;
        if (c.img_kind == MMHIP_IMG_BEIT && P > 224) return MMHIP_E_INVALID;          // the attention forward with a 2-D bias is instantiated up to 224 keys
        // ... and on the matrix cores only: the parity mode's vector-ALU attention (MMHIP_X3_FAST=0) has no bias form, so such a handle is refused here
        // instead of failing in every forward
        if (c.img_kind == MMHIP_IMG_BEIT && c.dtype == MMHIP_BF16X3 && env_int("MMHIP_X3_FAST", 1) == 0) return MMHIP_E_INVALID;
    }
    if (c.max_text_len > 128 || c.max_text_len < 1 || c.max_posts < 1 || c.max_posts > 1024) return MMHIP_E_INVALID;
    if (c.dtype != MMHIP_BF16 && c.dtype != MMHIP_F16 && c.dtype != MMHIP_BF16X3) return MMHIP_E_INVALID;
    if (c.num_labels < 1 || c.num_labels > 64 || c.proj_dim < 1 || c.proj_dim > 1024) return MMHIP_E_INVALID;
    if (c.txt_kind == MMHIP_TXT_XLMR && c.max_pos < c.max_text_len + c.pad_id + 1) return MMHIP_E_INVALID;
    if (c.txt_kind == MMHIP_TXT_BERT && c.max_pos < c.max_text_len) return MMHIP_E_INVALID;
    mmhip_engine* e = new (std::nothrow) mmhip_engine();
    if (!e) return MMHIP_E_INVALID;
    e->cfg = c;
    read_x3_env(*e);
    build_layout(*e);
    build_workspace(*e);
    *out = e;
    return 0;
}
void mmhip_destroy(mmhip_handle h) {
    if (!h) return;
    if (h->side) {
        (void)hipStreamSynchronize(h->side);
        for (hipEvent_t ev : {h->ev_fork, h->ev_vit, h->ev_ready[0], h->ev_ready[1], h->ev_tn[0], h->ev_tn[1], h->ev_layer[0], h->ev_layer[1], h->ev_opt})
            if (ev) (void)hipEventDestroy(ev);
        for (auto sv : h->side_vit) if (sv) (void)hipStreamSynchronize(sv);      // pooled streams: drained, not destroyed
        for (auto ev : h->span_ev) if (ev) (void)hipEventDestroy(ev);
    }
    for (auto& ev : h->evs) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    delete h;
}
int mmhip_param_count(mmhip_handle h) { return h ? (int)h->params.size() : MMHIP_E_INVALID; }
int mmhip_param_info_at(mmhip_handle h, int i, mmhip_param_info* out) {
    if (!h || !out || i < 0 || i >= (int)h->params.size()) return MMHIP_E_INVALID;
    *out = h->params[i];
    return 0;
}
uint64_t mmhip_buffer_numel(mmhip_handle h, int buffer) { return !h ? 0 : (buffer == 0 ? h->n_frozen : h->n_train); }
uint64_t mmhip_workspace_bytes(mmhip_handle h) { return h ? h->ws_need : 0; }
int mmhip_reserve_itc_global(mmhip_handle h, int max_world) {
    if (!h || max_world < 0) return MMHIP_E_INVALID;
    if (h->ws || !h->is_late()) return MMHIP_E_STATE;          // the workspace is sized before it is bound
    mmhip_engine& e = *h;
    const size_t Bm = e.cfg.max_posts, E = e.cfg.proj_dim, Gm = (size_t)max_world * Bm;
    if (max_world > 1 && Gm > (size_t)ITC_GLOBAL_MAX_G) return MMHIP_E_INVALID;
    e.itc_max_world = max_world > 1 ? max_world : 0;
    e.itc_world = 1; e.itc_rank = 0;
    e.ws_need = e.ws_base;
    if (!e.itc_max_world) return 0;
    Carver w;
    w.off = e.ws_base;
    e.h_g_txt = w.take(Gm * E * 4); e.h_g_img = w.take(Gm * E * 4); e.h_g_rowlse = w.take(Gm * 4); e.h_g_collse = w.take(Gm * 4); e.h_g_loss = w.take(16);
    e.h_g_dtn = w.take(Bm * E * 4); e.h_g_din = w.take(Bm * E * 4); e.h_g_ws = w.take(itc_global_ws_floats((int)Gm, (int)Bm) * 4);
    e.ws_need = w.off;
    return 0;
}
int mmhip_set_itc_global(mmhip_handle h, int world, int rank) {
    if (!h || world < 1 || rank < 0 || rank >= world) return MMHIP_E_INVALID;
    if (!h->is_late()) return MMHIP_E_STATE;
    if (world > 1 && world > h->itc_max_world) return MMHIP_E_CAPACITY;
    h->itc_world = world; h->itc_rank = rank;
    return 0;
}
int mmhip_itc_gather_buffers(mmhip_handle h, void** txt_local, void** img_local, void** txt_all, void** img_all) {
    if (!h || !h->ws || !h->itc_max_world || !h->is_late()) return MMHIP_E_STATE;
    const mmhip_engine& e = *h;
    if (txt_local) *txt_local = e.ws + e.h_txt_n;
    if (img_local) *img_local = e.ws + e.h_img_n;
    if (txt_all) *txt_all = e.ws + e.h_g_txt;
    if (img_all) *img_all = e.ws + e.h_g_img;
    return 0;
}
int mmhip_bind(mmhip_handle h, float* frozen, float* train, float* train_grad, void* workspace, uint64_t workspace_bytes) {
    if (!h || !frozen || !train || !workspace || !h->is_late()) return MMHIP_E_INVALID;
    if (workspace_bytes < h->ws_need) return MMHIP_E_CAPACITY;
    if (((uintptr_t)frozen | (uintptr_t)train | (uintptr_t)train_grad | (uintptr_t)workspace) & 255) return MMHIP_E_INVALID;
    h->frozen = frozen; h->train = train; h->grad = train_grad; h->ws = (char*)workspace; h->ws_bytes = workspace_bytes;
    h->fwd_done = false;
    return 0;
}
int mmhip_refresh_weights(mmhip_handle h, int which, void* stream) {
    if (!h || !h->ws) return MMHIP_E_STATE;
    hipStream_t s = (hipStream_t)stream;
    mmhip_engine& e = *h;
    if ((which & 1) && e.is_text()) return MMHIP_E_STATE;          // no image tower, no frozen buffer (mmhip_txt_refresh_weights refreshes the text tower)
    if (e.is_image()) return MMHIP_E_STATE;                         // (mmhip_img_refresh_weights)
    if (which & 1) {
        for (int l = 0; l < e.cfg.layers_img; ++l) {
            if (e.beit()) CHECK_RC(refresh_layer_beit(e, l, s));
            else CHECK_RC(refresh_layer(e, e.frozen, e.vit[l], e.vit_w16[l], false, s, e.Hv(), e.Iv()));
        }
        CHECK_RC(refresh_patch(e, e.frozen, s));
    }
    if (which & 2)
        for (int l = 0; l < e.cfg.layers_txt; ++l)
            CHECK_RC(refresh_layer(e, e.train, e.txt[l], e.txt_w16[l], true, s, e.cfg.hidden, e.cfg.inter));
    return 0;
}

int mmhip_forward(mmhip_handle h, const int64_t* ids, const int64_t* mask, const float* pixels, const int64_t* tim_ids,
                  const int64_t* tim_mask, int B, int T, int train, uint64_t seed, float* out_cls, float* logits_per_text,
                  float* out_tim, float* mm_features, void* stream) {
    if (!h || !h->ws || !h->is_late()) return MMHIP_E_STATE;          // (a text-only handle has mmhip_txt_forward, an image-only one mmhip_img_forward)
    if (!ids || !mask || B < 1 || T < 1) return MMHIP_E_INVALID;
    if ((tim_ids == nullptr) != (tim_mask == nullptr)) return MMHIP_E_INVALID;
    mmhip_engine& e = *h;
    // aspect-att has no ITM pass: the reference's second mm_fusion call (models/mm_late.py:181) comes without the pooled inputs and raises
    if (e.aspect() && tim_ids) return MMHIP_E_INVALID;
    const bool imported = pixels == nullptr;           // image tower outputs come from the caller's cache (mmhip_vision_import)
    if (imported && e.vision_ready_B != B) return MMHIP_E_STATE;
    e.vision_ready_B = 0;
    if (B > e.cfg.max_posts || T > e.cfg.max_text_len) return MMHIP_E_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    e.B = B; e.T = T; e.itm = tim_ids != nullptr; e.Bt = e.itm ? 2 * B : B; e.train_mode = train != 0; e.seed = seed;
    e.fwd_done = false; e.bwd_begun = false;
    const size_t nb = (size_t)B * T * 8;
    // token ids are clamped into the word table on their way into the engine's copy (launch_copy_ids_clamped: why)
    CHECK_HIP(launch_copy_ids_clamped(ids, e.wsp<int64_t>(e.ids_all), (size_t)B * T, e.cfg.vocab, e.bad_index, s));
    CHECK_HIP(hipMemcpyAsync(e.ws + e.mask_all, mask, nb, hipMemcpyDeviceToDevice, s));
    if (e.itm) {
        CHECK_HIP(launch_copy_ids_clamped(tim_ids, e.wsp<int64_t>(e.ids_all) + (size_t)B * T, (size_t)B * T, e.cfg.vocab, e.bad_index, s));
        CHECK_HIP(hipMemcpyAsync(e.ws + e.mask_all + nb, tim_mask, nb, hipMemcpyDeviceToDevice, s));
    }
    CHECK_RC(side_init(e));
    if (e.part[0] < 0) {
        // MMHIP_PART: "txt,vit" forces a split, "0" turns the partition off; default: chosen per forward (choose_partition)
        e.part[0] = e.part[1] = 0; e.part_auto = true;
        if (const char* v = getenv("MMHIP_PART")) {
            int a = 0, b = 0;
            e.part_auto = false;
            if (sscanf(v, "%d,%d", &a, &b) == 2 && a > 0 && b > 0) { e.part[0] = a; e.part[1] = b; }
        }
    }
    const bool can_part = !imported && use_side(e) && (e.dt() == DT_BF16 || e.dt() == DT_F16);
    e.cur_part[0] = e.cur_part[1] = 0;
    if (can_part && e.part_auto) choose_partition(e);
    else if (can_part && e.part[0] > 0) { e.cur_part[0] = e.part[0]; e.cur_part[1] = e.part[1]; }
    if (use_side(e)) {
        // the frozen image tower does not depend on the text tower: run it on the side stream, join before the heads
        CHECK_HIP(hipEventRecord(e.ev_fork, s));
        CHECK_RC(e.span(0, s));
        const bool vit_longer = (double)e.B * e.P() * e.cfg.layers_img > (double)e.Bt * e.T * e.cfg.layers_txt;     // rows x layers of equal width
        e.vit_is_long = vit_longer;
        hipStream_t sv = e.side_vit[vit_longer ? 1 : 0];
        if (!imported) {
            CHECK_HIP(hipStreamWaitEvent(sv, e.ev_fork, 0));
            CHECK_RC(vit_forward(e, pixels, sv));
            CHECK_RC(e.span(1, sv));
            CHECK_HIP(hipEventRecord(e.ev_vit, sv));
        }
        CHECK_RC(text_forward(e, s));
        CHECK_RC(e.span(2, s));
        if (!imported) CHECK_HIP(hipStreamWaitEvent(s, e.ev_vit, 0));
    } else {
        CHECK_RC(e.span(0, s));
        if (!imported) CHECK_RC(vit_forward(e, pixels, s));
        CHECK_RC(e.span(1, s));
        CHECK_RC(text_forward(e, s));
        CHECK_RC(e.span(2, s));
    }
    CHECK_RC(heads_forward(e, out_cls, logits_per_text, out_tim, mm_features, s));
    CHECK_RC(e.span(3, s));
    e.fwd_done = true;
    return 0;
}

// ---- image-tower output cache (the tower is frozen and dropout-free: its output is a pure function of the pixels)
namespace {
__global__ __launch_bounds__(256) void vision_copy_kernel(int to_cache, const int64_t* __restrict__ slots, char* cache, uint64_t rec_bytes,
                                                          uint64_t cache_records, char* v_out, char* vpool, uint32_t tok_bytes, uint32_t pool_bytes) {
    const int64_t slot = slots[blockIdx.y];
    if (slot < 0 || (uint64_t)slot >= cache_records) return;
    char* rec = cache + (uint64_t)slot * rec_bytes;
    char* tok = v_out + (size_t)blockIdx.y * tok_bytes;
    char* pool = vpool + (size_t)blockIdx.y * pool_bytes;
    const uint32_t n16 = (tok_bytes + pool_bytes) / 16, t16 = tok_bytes / 16;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) {
        uint4* live = reinterpret_cast<uint4*>(i < t16 ? tok + (size_t)i * 16 : pool + (size_t)(i - t16) * 16);
        uint4* kept = reinterpret_cast<uint4*>(rec + (size_t)i * 16);
        if (to_cache) *kept = *live;
        else *live = *kept;
    }
}
int vision_copy(mmhip_engine& e, int to_cache, const int64_t* slots, void* cache, uint64_t cache_records, int B, hipStream_t s) {
    const int P = e.P(), H = e.Hv();
    const uint32_t tok_bytes = (uint32_t)(P * H * e.esz()), pool_bytes = (uint32_t)H * 4;
    if (tok_bytes % 16 || pool_bytes % 16) return MMHIP_E_INVALID;
    hipLaunchKernelGGL(vision_copy_kernel, dim3(16, B), dim3(256), 0, s, to_cache, slots, (char*)cache, mmhip_vision_record_bytes(&e), cache_records,
                       e.ws + e.v_out, (char*)e.wsp<float>(e.h_vpool), tok_bytes, pool_bytes);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : (int)err;
}
}  // namespace
uint64_t mmhip_vision_record_bytes(mmhip_handle h) {
    if (!h) return 0;
    const uint64_t P = (uint64_t)h->P();
    return (P * h->Hv() * h->esz() + (uint64_t)h->Hv() * 4 + 255) & ~255ull;
}
int mmhip_vision_export(mmhip_handle h, const int64_t* slots, void* cache, uint64_t cache_records, void* stream) {
    if (!h || !h->ws || !h->fwd_done || !h->is_late()) return MMHIP_E_STATE;
    if (!slots || !cache || ((uintptr_t)cache & 15)) return MMHIP_E_INVALID;
    return vision_copy(*h, 1, slots, cache, cache_records, h->B, (hipStream_t)stream);
}
int mmhip_vision_import(mmhip_handle h, const int64_t* slots, const void* cache, uint64_t cache_records, int B, void* stream) {
    if (!h || !h->ws || !h->is_late()) return MMHIP_E_STATE;
    if (!slots || !cache || ((uintptr_t)cache & 15) || B < 1) return MMHIP_E_INVALID;
    if (B > h->cfg.max_posts) return MMHIP_E_CAPACITY;
    CHECK_RC(vision_copy(*h, 0, slots, const_cast<void*>(cache), cache_records, B, (hipStream_t)stream));
    h->vision_ready_B = B;
    return 0;
}

int mmhip_loss(mmhip_handle h, const int64_t* onehot, const float* class_w, const int64_t* lbl_tim, float w_cls, float w_itc,
               float w_itm, float* loss, int* n_correct, void* stream) {
    if (!h || !h->fwd_done || !h->is_late()) return MMHIP_E_STATE;
    if (!onehot) return MMHIP_E_INVALID;
    mmhip_engine& e = *h;
    if (w_itm != 0.f && (!e.itm || !lbl_tim)) return MMHIP_E_INVALID;
    if (w_itc != 0.f && !e.itc_done) return MMHIP_E_STATE;
    hipStream_t s = (hipStream_t)stream;
    // global-batch ITC: a training forward whose normalised rows the caller has gathered (MMHIP_CB_GATHER_ITC / mmhip_itc_gather_buffers) takes its
    // ITC term from the G x G logits of all ranks' posts; evaluation and world 1 keep the rank's own [B, B] block
    const bool glob = e.itc_world > 1 && e.train_mode && w_itc != 0.f;
    LossArgs a{};
    a.out_cls = e.wsp<float>(e.h_out_cls); a.onehot = onehot; a.class_w = class_w;
    if (glob) {
        ItcGlobalArgs ga{e.wsp<float>(e.h_g_txt), e.wsp<float>(e.h_g_img), e.train + e.logit_scale, nullptr, e.wsp<float>(e.h_g_rowlse),
                         e.wsp<float>(e.h_g_collse), e.wsp<float>(e.h_g_loss), e.wsp<float>(e.h_g_ws), e.itc_world * e.B, e.cfg.proj_dim};
        CHECK_HIP(launch_itc_global_fwd(ga, s));
        a.itc_global_loss = ga.loss;
    }
    a.logits_per_text = w_itc != 0.f && !glob ? e.wsp<float>(e.h_logits) : nullptr;
    a.out_tim = w_itm != 0.f ? e.wsp<float>(e.h_out_tim) : nullptr; a.lbl_tim = lbl_tim;
    a.w_cls = w_cls; a.w_itc = w_itc; a.w_itm = w_itm;
    a.loss = e.wsp<float>(e.h_loss);
    a.d_out_cls = e.wsp<float>(e.h_d_out_cls);
    a.d_logits = w_itc != 0.f && !glob ? e.wsp<float>(e.h_d_logits) : nullptr;
    a.d_out_tim = w_itm != 0.f ? e.wsp<float>(e.h_d_out_tim) : nullptr;
    a.n_correct = n_correct;
    a.B = e.B; a.C = e.cfg.num_labels;
    CHECK_HIP(launch_loss(a, s));
    if (loss) CHECK_HIP(hipMemcpyAsync(loss, a.loss, 16, hipMemcpyDeviceToDevice, s));
    e.bd_out_cls = a.d_out_cls; e.bd_logits = a.d_logits; e.bd_out_tim = a.d_out_tim; e.bd_feats = nullptr;
    e.bd_itc_global = glob; e.bd_w_itc = w_itc;
    return 0;
}

int mmhip_num_backward_stages(mmhip_handle h) { return h ? h->nl() + 2 : MMHIP_E_INVALID; }

int mmhip_stage_grad_range(mmhip_handle h, int stage, uint64_t* begin, uint64_t* end) {
    if (!h || !begin || !end || stage < 0 || stage > h->nl() + 1) return MMHIP_E_INVALID;
    const mmhip_engine& e = *h;
    if (stage == 0) { *begin = e.heads_begin; *end = e.heads_end; }
    else if (stage <= e.nl()) { const LayerOff& o = e.lay()[e.nl() - stage]; *begin = o.begin; *end = o.end; }
    else { *begin = e.emb_begin; *end = e.emb_end; }
    return 0;
}

int mmhip_backward_begin(mmhip_handle h, const float* d_out_cls, const float* d_logits, const float* d_out_tim, const float* d_feats, void* stream) {
    if (!h || !h->fwd_done || !h->grad) return MMHIP_E_STATE;
    mmhip_engine& e = *h;
    if (unsigned* f = guard_flag(e)) CHECK_HIP(hipMemsetAsync(f, 0, 4, (hipStream_t)stream));      // the step guard's flag belongs to one backward
    if (d_out_cls || d_logits || d_out_tim || d_feats) {
        if (!d_out_cls) return MMHIP_E_INVALID;
        e.bd_out_cls = d_out_cls; e.bd_logits = d_logits; e.bd_out_tim = d_out_tim; e.bd_feats = d_feats;
        e.bd_itc_global = false;          // explicit output gradients (autograd binding): d_logits is the rank's own [B, B] block
    } else if (!e.bd_out_cls) {
        return MMHIP_E_STATE;      // no mmhip_loss before, and no explicit gradients
    }
    e.bwd_begun = true;
    e.tn_pending[0] = e.tn_pending[1] = false;
    return side_init(e);
}
int mmhip_backward_stage(mmhip_handle h, int stage, void* stream) {
    if (!h || !h->bwd_begun) return MMHIP_E_STATE;
    mmhip_engine& e = *h;
    hipStream_t s = (hipStream_t)stream;
    const int L = e.nl();
    if (e.is_image()) {
        if (stage == 0) return img_head_backward(e, s);
        if (stage >= 1 && stage <= L) return image_layer_backward(e, L - stage, s);
        if (stage == L + 1) return img_embed_backward(e, s);
        return MMHIP_E_INVALID;
    }
    if (stage == 0) return e.is_text() ? txt_head_backward(e, s) : heads_backward(e, s);
    if (stage >= 1 && stage <= L) return text_layer_backward(e, L - stage, s);
    if (stage == L + 1) return embed_backward(e, s);
    return MMHIP_E_INVALID;
}
int mmhip_backward_join_stage(mmhip_handle h, int stage, void* stream) {
    if (!h || !h->bwd_begun) return MMHIP_E_STATE;
    mmhip_engine& e = *h;
    const int L = e.nl();
    if (stage < 1 || stage > L) return 0;
    return join_set(e, (L - stage) & 1, (hipStream_t)stream);
}
int mmhip_backward_finish(mmhip_handle h, void* stream) {
    if (!h || !h->bwd_begun) return MMHIP_E_STATE;
    return backward_finish(*h, (hipStream_t)stream);
}
int mmhip_backward(mmhip_handle h, const float* d_out_cls, const float* d_logits, const float* d_out_tim, const float* d_feats, void* stream) {
    CHECK_RC(mmhip_backward_begin(h, d_out_cls, d_logits, d_out_tim, d_feats, stream));
    const int n = mmhip_num_backward_stages(h);
    for (int st = 0; st < n; ++st)
        CHECK_RC(mmhip_backward_stage(h, st, stream));
    return mmhip_backward_finish(h, stream);
}

int mmhip_set_nonfinite_counter(uint32_t* device_counter) {
    if ((uintptr_t)device_counter & 3) return MMHIP_E_INVALID;
    g_nonfinite = device_counter;
    g_skip = nullptr;
    return 0;
}
int mmhip_set_step_guard(uint32_t* device_words2) {
    if ((uintptr_t)device_words2 & 3) return MMHIP_E_INVALID;
    g_nonfinite = device_words2;
    g_skip = device_words2 ? device_words2 + 1 : nullptr;
    return 0;
}
int mmhip_set_guard(mmhip_handle h, uint32_t* device_words2) {
    if (!h || ((uintptr_t)device_words2 & 3)) return MMHIP_E_INVALID;
    h->guard = device_words2;
    return 0;
}
void* mmhip_side_stream(mmhip_handle h) {
    if (!h) return nullptr;
    if (side_init(*h)) return nullptr;
    return use_side(*h) ? (void*)h->side : nullptr;
}
int mmhip_set_index_counter(mmhip_handle h, uint32_t* device_word) {
    if (!h || ((uintptr_t)device_word & 3)) return MMHIP_E_INVALID;
    h->bad_index = device_word;
    return 0;
}
int mmhip_set_backward_products(mmhip_handle h, int products) {
    if (!h || products < 1 || products > 3) return MMHIP_E_INVALID;
    if (h->cfg.dtype != MMHIP_BF16X3 || !h->px) return products == 3 ? 0 : MMHIP_E_STATE;      // the 16-bit modes have one product; round 3's copy form has three
    h->bwd_np = products;
    return 0;
}
int mmhip_set_drop_path(mmhip_handle h, float rate) {
    if (!h || !h->is_late() || !h->beit() || !(rate >= 0.f) || rate >= 1.f) return MMHIP_E_INVALID;
    h->drop_path = rate;
    return 0;
}
// global-norm gradient clipping of the fused steps: armed with a threshold and the caller's state block, disarmed by NULL or max_norm <= 0
int mmhip_set_grad_clip(mmhip_handle h, float max_norm, void* clip_state) {
    if (!h || std::isnan(max_norm) || std::isinf(max_norm) || ((uintptr_t)clip_state & 15)) return MMHIP_E_INVALID;
    const bool arm = clip_state && max_norm > 0.f;
    h->clip_state = arm ? clip_state : nullptr;
    h->clip_max = arm ? max_norm : 0.f;
    return 0;
}
int mmhip_set_loss_scale(mmhip_handle h, float loss_scale) {
    if (!h || !(loss_scale >= 0.f)) return MMHIP_E_INVALID;
    h->cfg.loss_scale = loss_scale;
    return 0;
}

static int adamw_impl(float* p, float* g, float* m, float* v, uint64_t n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int step, float grad_scale, int zero_grad, void* stream, unsigned* g_nonfinite, const unsigned* g_skip,
                      const void* clip_state = nullptr) {
    if (!p || !g || !m || !v || step < 1) return MMHIP_E_INVALID;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return MMHIP_E_INVALID;
    if ((uintptr_t)clip_state & 15) return MMHIP_E_INVALID;
    AdamWArgs a = adamw_args(lr, beta1, beta2, eps, weight_decay, step, grad_scale, zero_grad, g_nonfinite, g_skip);
    a.p = p; a.g = g; a.m = m; a.v = v; a.n = n;
    a.clip = static_cast<const float*>(clip_state);          // word 0 of the block: the coefficient
    CHECK_HIP(launch_adamw(a, (hipStream_t)stream));
    return 0;
}
int mmhip_adamw(float* p, float* g, float* m, float* v, uint64_t n, float lr, float beta1, float beta2, float eps,
                float weight_decay, int step, float grad_scale, int zero_grad, void* stream) {
    return adamw_impl(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, zero_grad, stream, g_nonfinite, g_skip);
}
int mmhip_adamw_guarded(float* p, float* g, float* m, float* v, uint64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, float grad_scale, int zero_grad, void* stream, uint32_t* guard_words2) {
    if ((uintptr_t)guard_words2 & 3) return MMHIP_E_INVALID;
    return adamw_impl(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, zero_grad, stream, guard_words2, guard_words2 ? guard_words2 + 1 : nullptr);
}
int mmhip_adamw_clipped(float* p, float* g, float* m, float* v, uint64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, float grad_scale, int zero_grad, void* stream, uint32_t* guard_words2, const void* clip_state) {
    if ((uintptr_t)guard_words2 & 3) return MMHIP_E_INVALID;
    return adamw_impl(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, zero_grad, stream, guard_words2, guard_words2 ? guard_words2 + 1 : nullptr,
                      clip_state);
}

int mmhip_set_row_state(mmhip_handle h, uint8_t* row_state) {
    if (!h) return MMHIP_E_INVALID;
    if ((uintptr_t)row_state & 3) return MMHIP_E_INVALID;
    h->word_row_state = row_state;
    return 0;
}

static int adamw_rows_impl(float* p, float* g, float* m, float* v, int rows, int width, uint8_t* row_state, float lr, float beta1, float beta2,
                           float eps, float weight_decay, int step, float grad_scale, int zero_grad, void* stream, unsigned* g_nonfinite, const unsigned* g_skip,
                           const void* clip_state = nullptr) {
    if (!p || !g || !m || !v || !row_state || step < 1 || rows < 0 || width <= 0 || width % 4) return MMHIP_E_INVALID;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return MMHIP_E_INVALID;
    if ((uintptr_t)clip_state & 15) return MMHIP_E_INVALID;
    AdamWArgs a = adamw_args(lr, beta1, beta2, eps, weight_decay, step, grad_scale, zero_grad, g_nonfinite, g_skip);
    a.p = p; a.g = g; a.m = m; a.v = v; a.n = (size_t)rows * width;
    a.clip = static_cast<const float*>(clip_state);
    CHECK_HIP(launch_adamw_rows(a, rows, width, row_state, (hipStream_t)stream));
    return 0;
}
int mmhip_adamw_rows(float* p, float* g, float* m, float* v, int rows, int width, uint8_t* row_state, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, float grad_scale, int zero_grad, void* stream) {
    return adamw_rows_impl(p, g, m, v, rows, width, row_state, lr, beta1, beta2, eps, weight_decay, step, grad_scale, zero_grad, stream, g_nonfinite, g_skip);
}
int mmhip_adamw_rows_guarded(float* p, float* g, float* m, float* v, int rows, int width, uint8_t* row_state, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int step, float grad_scale, int zero_grad, void* stream, uint32_t* guard_words2) {
    if ((uintptr_t)guard_words2 & 3) return MMHIP_E_INVALID;
    return adamw_rows_impl(p, g, m, v, rows, width, row_state, lr, beta1, beta2, eps, weight_decay, step, grad_scale, zero_grad, stream, guard_words2,
                           guard_words2 ? guard_words2 + 1 : nullptr);
}
int mmhip_adamw_rows_clipped(float* p, float* g, float* m, float* v, int rows, int width, uint8_t* row_state, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int step, float grad_scale, int zero_grad, void* stream, uint32_t* guard_words2,
                             const void* clip_state) {
    if ((uintptr_t)guard_words2 & 3) return MMHIP_E_INVALID;
    return adamw_rows_impl(p, g, m, v, rows, width, row_state, lr, beta1, beta2, eps, weight_decay, step, grad_scale, zero_grad, stream, guard_words2,
                           guard_words2 ? guard_words2 + 1 : nullptr, clip_state);
}

static int step_backward_update(mmhip_handle h, int use_itc, int use_itm, float* adam_m, float* adam_v, float lr, float beta1, float beta2, float eps,
                                float weight_decay, int step, float grad_scale, void* stream, mmhip_exchange_cb cb, void* user);

// The range walk of a fused step, written once: the merged [begin, end) ranges of the active gradient groups in address order, as the dense part of
// each (below the word table) and whether the word table is among them.  layer_done (may be null): text layers whose optimizer has already run beside
// the backward are skipped.  The AdamW launches, the norm of an armed clip and the check ahead of an armed step all go over this list.
struct StepRange { uint64_t b, e; };
static void collect_step_ranges(const mmhip_engine& e, int use_itc, int use_itm, const std::vector<char>* layer_done, std::vector<StepRange>& dense, bool& rows_due) {
    const bool act[6] = {false, use_itc != 0, use_itm != 0, e.cfg.fusion == MMHIP_FUSION_ATTENTION, true, false};
    const uint64_t w0 = e.is_image() ? e.n_train : e.t_word;          // (no word table in an image-only handle)
    const std::vector<LayerOff>& lay = e.lay();
    const int L = e.nl();
    uint64_t rb = 0, re = 0;
    bool open = false;
    dense.clear();
    rows_due = false;
    auto flush = [&]() {
        if (!open || re <= rb) return;
        const uint64_t dense_end = re < w0 ? re : w0;
        if (dense_end > rb) dense.push_back(StepRange{rb, dense_end});
        if (re > w0) rows_due = true;          // the word table goes last: under data parallelism its rows are still travelling
    };
    auto in_layer = [&](uint64_t off) {          // a text layer whose optimizer has already run (beside the backward)
        if (!layer_done) return false;
        for (int l = 0; l < L; ++l) if ((*layer_done)[l] && off >= lay[l].begin && off < lay[l].end) return true;
        return false;
    };
    for (const auto& p : e.params) {
        if (p.buffer != 1 || !act[p.group] || in_layer(p.offset)) continue;
        const uint64_t b = p.offset, en = p.offset + ((p.numel + 3) & ~(uint64_t)3);
        if (open && b == re) { re = en; continue; }
        flush();
        rb = b; re = en; open = true;
    }
    flush();
}
// An armed clip's refusals are known from the layout and the handle: more merged ranges than one norm launch takes, a word table without its row
// flags.  Asked before the step's forward, so that a refusal enqueues nothing (as the data-parallel refusal does).
static int clip_step_check(const mmhip_engine& e, int use_itc, int use_itm) {
    if (!e.clip_state) return 0;
    std::vector<StepRange> dense;
    bool rows_due = false;
    collect_step_ranges(e, use_itc, use_itm, nullptr, dense, rows_due);
    if (dense.size() > (size_t)GRADNORM_MAX_SEGMENTS || (rows_due && !e.word_row_state)) return MMHIP_E_STATE;
    return 0;
}

// One fused training step, enqueued natively (no per-stage host round trips): forward (train mode) -> loss -> backward ->
// AdamW over the ranges that receive gradients for this flag set (torch skips `grad is None` tensors) ->
// 16-bit weight refresh.  Single-rank form of MMLate_Model.train_step; a data-parallel caller keeps the staged calls.
static int train_step_impl(mmhip_handle h, const int64_t* ids, const int64_t* mask, const float* pixels, const int64_t* tim_ids,
                           const int64_t* tim_mask, const int64_t* lbl_tim, const int64_t* onehot, const float* class_w, int B, int T,
                           uint64_t seed, int use_itc, int use_itm, float w_cls, float w_itc, float w_itm, float* adam_m, float* adam_v,
                           float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float* loss,
                           int* n_correct, void* stream, mmhip_exchange_cb cb, void* user) {
    if (!h || !h->ws || !h->grad) return MMHIP_E_STATE;
    if (!adam_m || !adam_v || !onehot || step < 1) return MMHIP_E_INVALID;
    if (use_itm && (!tim_ids || !lbl_tim)) return MMHIP_E_INVALID;
    mmhip_engine& e = *h;
    if (e.aspect() && (use_itm || tim_ids)) return MMHIP_E_INVALID;      // models/mm_late.py:181 (mmhip_forward)
    CHECK_RC(clip_step_check(e, use_itc, use_itm));
    e.skip_itc = !use_itc;
    const int rf = mmhip_forward(h, ids, mask, pixels, use_itm ? tim_ids : nullptr, use_itm ? tim_mask : nullptr, B, T, 1, seed, nullptr, nullptr,
                                 nullptr, nullptr, stream);
    e.skip_itc = false;
    if (rf) return rf;
    if (e.itc_world > 1 && use_itc) {
        // global-batch ITC: the local rows are normalised; the caller gathers every rank's (mmhip_itc_gather_buffers) and orders the
        // collectives before what follows in `stream`.  Without a callback nobody can fill the gathered rows
        if (!cb) return MMHIP_E_STATE;
        CHECK_RC(cb(user, MMHIP_CB_GATHER_ITC));
    }
    CHECK_RC(mmhip_loss(h, onehot, class_w, use_itm ? lbl_tim : nullptr, w_cls, use_itc ? w_itc : 0.f, use_itm ? w_itm : 0.f, loss, n_correct, stream));
    return step_backward_update(h, use_itc, use_itm, adam_m, adam_v, lr, beta1, beta2, eps, weight_decay, step, grad_scale, stream, cb, user);
}

// second half of a fused step, shared by the late-fusion and the text-only handle: backward, per-layer AdamW + operand refresh beside it, the
// remaining dense ranges, the row-lazy word table.  On entry the forward has run and the output gradients are in the handle.
static int step_backward_update(mmhip_handle h, int use_itc, int use_itm, float* adam_m, float* adam_v, float lr, float beta1, float beta2, float eps,
                                float weight_decay, int step, float grad_scale, void* stream, mmhip_exchange_cb cb, void* user) {
    mmhip_engine& e = *h;
    // Backward.  With the side stream on, each text layer's AdamW and 16-bit weight refresh follow its weight-gradient GEMM on the
    // SIDE stream, beside the activation-gradient chain of the layers below (an HBM-bound kernel next to MFMA-bound ones) instead
    // of after the whole backward; the layer's fp32 LayerNorm weights and transposed 16-bit copies are read by its own backward
    // kernels on the caller's stream, so the side stream first waits for the event recorded behind them.
    hipStream_t s = (hipStream_t)stream;
    // f16 with the step guard armed: a void step is only known when the backward has reached the embeddings, so every AdamW waits for it
    unsigned* gc = guard_counter(e);
    unsigned* gf = guard_flag(e);
    // global-norm clipping armed: the coefficient is known only when the whole gradient is, so -- by the same rule -- every AdamW waits for the backward
    const void* clip = e.clip_state;
    const int early = ((e.dt() == DT_F16 && gf) || clip) ? 0 : env_int("MMHIP_EARLY_ADAMW", 1);          // read per step: tests compare both orders in one process
    if (clip && !getenv("MMHIP_EARLY_ADAMW")) {
        static bool told = false;
        if (!told && getenv("MMHIP_VERBOSE")) { fprintf(stderr, "[mmhip] gradient clipping armed: every AdamW launch follows the backward and the norm (no per-layer optimizer beside it)\n"); told = true; }
    }
    if (e.dt() == DT_F16 && gf && !getenv("MMHIP_EARLY_ADAMW")) {
        static bool told = false;
        if (!told && getenv("MMHIP_VERBOSE")) { fprintf(stderr, "[mmhip] f16 with the step guard armed: every AdamW launch follows the backward (no per-layer optimizer beside it)\n"); told = true; }
    }
    CHECK_RC(mmhip_backward_begin(h, nullptr, nullptr, nullptr, nullptr, stream));
    const int L = e.nl();          // text layers; an image-only handle: its image layers
    const std::vector<LayerOff>& lay = e.lay();
    const std::vector<LayerW16>& lay16 = e.lay_w16();
    const int lH = e.is_image() ? e.Hv() : e.cfg.hidden, lI = e.is_image() ? e.Iv() : e.cfg.inter;
    // data-parallel form (cb): the callback is told about stage st-1 once stage st is enqueued and st-1's weight gradients are ordered in the
    // caller's stream -- its collective travels while the stages below compute.  The layer optimizers wait for the gradient exchange: PER BUCKET
    // (round 5).  When the callback answers MMHIP_CB_BUCKET -- "the collective that carries every stage since the last such answer has been
    // started" -- the side stream is made to wait for that collective (on_stage(MMHIP_CB_WAIT_BUCKET): the caller waits on mmhip_side_stream) and
    // the AdamW + operand refresh of the text layers it carries follow on the side stream, beside the stages below, as in the single-rank step;
    // before round 5 every layer's optimizer sat behind ONE barrier after the last all-reduce (MMHIP_CB_WAIT_DENSE), which made the N > 1 step
    // longer than the N = 1 step before any wire time.  Ranges that are not text layers (heads, embeddings) and the last, unflushed bucket keep
    // that barrier.
    const bool layer_opt = early && use_side(e) && !cb;
    const bool bucket_opt = early && use_side(e) && cb;
    bool opt_pending = false, dense_by_caller = false;
    std::vector<char> layer_done((size_t)(L > 0 ? L : 1), 0);
    std::vector<int> open_layers;          // text layers whose gradient stage lies in the bucket that is still open
    // text layer l on the side stream: its AdamW (adamw = false: the caller stepped it, MMHIP_CB_HANDLED), then its 16-bit operand refresh
    auto layer_update = [&](int l, bool adamw) -> int {
        const LayerOff& o = lay[l];
        if (adamw)
            CHECK_RC(adamw_impl(e.train + o.begin, e.grad + o.begin, adam_m + o.begin, adam_v + o.begin, o.end - o.begin, lr, beta1, beta2, eps, weight_decay,
                                step, grad_scale, 1, e.side, gc, gf));
        CHECK_RC(refresh_layer(e, e.train, o, lay16[l], true, e.side, lH, lI));
        layer_done[l] = adamw ? 1 : 2;          // 2: stepped by the caller, refreshed here
        return 0;
    };
    for (int st = 0; st < L + 2; ++st) {
        CHECK_RC(mmhip_backward_stage(h, st, stream));
        if (cb && st >= 1) {
            CHECK_RC(mmhip_backward_join_stage(h, st - 1, stream));
            const int r = cb(user, st - 1);
            if (r != 0 && r != MMHIP_CB_BUCKET) return r;
            if (st - 1 >= 1 && st - 1 <= L) open_layers.push_back(L - (st - 1));
            if (r == MMHIP_CB_BUCKET) {
                if (bucket_opt && !open_layers.empty()) {
                    // the side stream waits for the layers' backward kernels on `s` (they read the fp32 LayerNorm weights and the transposed
                    // operand copies that the optimizer and the refresh are about to overwrite) and, through the callback, for the collective
                    CHECK_HIP(hipEventRecord(e.ev_layer[0], s));
                    CHECK_HIP(hipStreamWaitEvent(e.side, e.ev_layer[0], 0));
                    const int w = cb(user, MMHIP_CB_WAIT_BUCKET);
                    if (w != 0 && w != MMHIP_CB_HANDLED) return w;
                    for (int l : open_layers) CHECK_RC(layer_update(l, w == 0));
                    CHECK_HIP(hipEventRecord(e.ev_opt, e.side));
                    opt_pending = true;
                }
                open_layers.clear();
            }
        }
        if (layer_opt && st >= 1 && st <= L) {
            const int l = L - st, set = l & 1;
            CHECK_HIP(hipEventRecord(e.ev_layer[set], s));
            CHECK_HIP(hipStreamWaitEvent(e.side, e.ev_layer[set], 0));
            CHECK_RC(layer_update(l, true));
            CHECK_HIP(hipEventRecord(e.ev_opt, e.side));
            opt_pending = true;
        }
    }
    CHECK_RC(mmhip_backward_finish(h, stream));
    if (opt_pending) CHECK_HIP(hipStreamWaitEvent(s, e.ev_opt, 0));
    if (cb) {
        CHECK_RC(cb(user, L + 1));                    // embedding stage: dense part + the row-sparse word-table exchange start
        // the dense exchanges are ordered before what follows in `stream`; MMHIP_CB_HANDLED: the caller also ran the dense optimizer itself
        // (reduce-scatter -> AdamW on its shard -> all-gather of the parameters: dist.ShardedBuckets) -- the dense AdamW launches below are skipped
        const int r = cb(user, MMHIP_CB_WAIT_DENSE);
        if (r == MMHIP_CB_HANDLED) dense_by_caller = true;
        else if (r) return r;
    }
    CHECK_RC(e.span(4, s));
    // merged [begin, end) ranges of the active gradient groups, in address order (text layers already stepped: skipped)
    const uint64_t w0 = e.is_image() ? e.n_train : e.t_word, V = (uint64_t)e.cfg.vocab, H = (uint64_t)e.cfg.hidden;      // (no word table in an image-only handle)
    std::vector<StepRange> dense;
    bool rows_due = false;
    collect_step_ranges(e, use_itc, use_itm, &layer_done, dense, rows_due);
    if (clip) {
        // (more than GRADNORM_MAX_SEGMENTS ranges, or a word table without row flags: clip_step_check refused the step before its forward)
        // the norm over exactly what is stepped below: the dense ranges and the word-table rows the backward flagged (an unflagged row's gradient is
        // zero by the row-lazy contract).  The flat gradient holds UNSCALED gradients in f16 as well (1 / gscale() is applied where they are written),
        // so the factor is AdamW's grad_scale and nothing else
        GradNormSegments sg{};
        for (const StepRange& r : dense) { sg.g[sg.count] = e.grad + r.b; sg.n[sg.count] = r.e - r.b; ++sg.count; }
        CHECK_HIP(launch_grad_clip(sg, rows_due ? e.grad + w0 : nullptr, rows_due ? (int)V : 0, (int)H, e.word_row_state, e.clip_max, grad_scale, gf, e.clip_state, s));
    }
    if (!dense_by_caller)
        for (const StepRange& r : dense)
            CHECK_RC(adamw_impl(e.train + r.b, e.grad + r.b, adam_m + r.b, adam_v + r.b, r.e - r.b, lr, beta1, beta2, eps, weight_decay, step, grad_scale, 1,
                                stream, gc, gf, clip));
    for (int l = 0; l < L; ++l)          // 16-bit GEMM operand copies of the layers stepped just now: no word-table dependence
        if (!layer_done[l]) CHECK_RC(refresh_layer(e, e.train, lay[l], lay16[l], true, s, lH, lI));
    if (e.is_image())          // the patch weight was stepped with the embeddings' range just now
        CHECK_RC(refresh_patch(e, e.train, s));
    if (rows_due) {
        if (cb) CHECK_RC(cb(user, MMHIP_CB_FINISH_ROWS));                 // the exchanged word rows are summed into the gradient
        if (!e.word_row_state) return MMHIP_E_STATE;
        CHECK_RC(adamw_rows_impl(e.train + w0, e.grad + w0, adam_m + w0, adam_v + w0, (int)V, (int)H, e.word_row_state, lr, beta1, beta2, eps,
                                    weight_decay, step, grad_scale, 1, stream, gc, gf, clip));
    }
    return e.span(5, s);
}

int mmhip_train_step(mmhip_handle h, const int64_t* ids, const int64_t* mask, const float* pixels, const int64_t* tim_ids,
                     const int64_t* tim_mask, const int64_t* lbl_tim, const int64_t* onehot, const float* class_w, int B, int T,
                     uint64_t seed, int use_itc, int use_itm, float w_cls, float w_itc, float w_itm, float* adam_m, float* adam_v,
                     float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float* loss,
                     int* n_correct, void* stream) {
    return train_step_impl(h, ids, mask, pixels, tim_ids, tim_mask, lbl_tim, onehot, class_w, B, T, seed, use_itc, use_itm, w_cls, w_itc, w_itm,
                           adam_m, adam_v, lr, beta1, beta2, eps, weight_decay, step, grad_scale, loss, n_correct, stream, nullptr, nullptr);
}
int mmhip_train_step_dp(mmhip_handle h, const int64_t* ids, const int64_t* mask, const float* pixels, const int64_t* tim_ids,
                        const int64_t* tim_mask, const int64_t* lbl_tim, const int64_t* onehot, const float* class_w, int B, int T,
                        uint64_t seed, int use_itc, int use_itm, float w_cls, float w_itc, float w_itm, float* adam_m, float* adam_v,
                        float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float* loss,
                        int* n_correct, void* stream, mmhip_exchange_cb on_stage, void* user) {
    if (!on_stage) return MMHIP_E_INVALID;
    // global-norm clipping needs the whole summed gradient before the first AdamW launch; here the word-table rows arrive after the dense optimizer
    // (and a sharded caller holds partial norms only): refused before anything is enqueued
    if (h && h->clip_state) return MMHIP_E_STATE;
    return train_step_impl(h, ids, mask, pixels, tim_ids, tim_mask, lbl_tim, onehot, class_w, B, T, seed, use_itc, use_itm, w_cls, w_itc, w_itm,
                           adam_m, adam_v, lr, beta1, beta2, eps, weight_decay, step, grad_scale, loss, n_correct, stream, on_stage, user);
}

// phase ends of the last step as milliseconds after the forward's fork (hipEvents on the streams the phases run on; no profiler):
// ms[0] image tower end, [1] text tower end, [2] forward end (heads), [3] backward end (all gradients and layer optimizers joined),
// [4] step end.  enable != 0 arms the events for the following steps; a phase that was not recorded reads -1.  Synchronises.
int mmhip_step_spans(mmhip_handle h, int enable, float* ms) {
    if (!h) return MMHIP_E_INVALID;
    mmhip_engine& e = *h;
    if (ms) {
        for (int i = 0; i < 5; ++i) ms[i] = -1.f;
        if (e.span_set[0]) {
            for (int i = 1; i < 6; ++i) {
                if (!e.span_set[i]) continue;
                CHECK_HIP(hipEventSynchronize(e.span_ev[i]));
                float t = 0.f;
                if (hipEventElapsedTime(&t, e.span_ev[0], e.span_ev[i]) == hipSuccess) ms[i - 1] = t;
            }
        }
    }
    e.spans_on = enable;
    if (!enable) for (int i = 0; i < 6; ++i) e.span_set[i] = false;
    return 0;
}
int mmhip_gemm_timing(mmhip_handle h, int enable, int reset, double* ms, uint64_t* launches, double* flops) {
    if (!h) return MMHIP_E_INVALID;
    mmhip_engine& e = *h;
    if (ms || launches || flops) {
        double tms = 0, tf = 0;
        for (size_t i = 0; i < e.ev_used; ++i) {
            CHECK_HIP(hipEventSynchronize(e.evs[i].b));
            float t = 0;
            CHECK_HIP(hipEventElapsedTime(&t, e.evs[i].a, e.evs[i].b));
            tms += t; tf += e.evs[i].flops;
        }
        if (ms) *ms = tms;
        if (launches) *launches = e.ev_used;
        if (flops) *flops = tf;
    }
    if (reset) e.ev_used = 0;
    e.timing = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return 0;
}

// per-shape table of the launches timed since the last reset (text, one line per (M, N, K, epilogue flags))
int mmhip_gemm_timing_by_shape(mmhip_handle h, char* out, uint64_t capacity) {
    if (!h || !out || capacity < 2) return MMHIP_E_INVALID;
    mmhip_engine& e = *h;
    struct Row { int M, N, K, flags, tile, cus; int n; double ms, flops; };
    std::vector<Row> rows;
    for (size_t i = 0; i < e.ev_used; ++i) {
        const auto& ev = e.evs[i];
        CHECK_HIP(hipEventSynchronize(ev.b));
        float t = 0;
        CHECK_HIP(hipEventElapsedTime(&t, ev.a, ev.b));
        Row* r = nullptr;
        for (auto& x : rows) if (x.M == ev.M && x.N == ev.N && x.K == ev.K && x.flags == ev.flags && x.tile == ev.tile && x.cus == ev.cus) { r = &x; break; }
        if (!r) { rows.push_back(Row{ev.M, ev.N, ev.K, ev.flags, ev.tile, ev.cus, 0, 0.0, 0.0}); r = &rows.back(); }
        r->n++; r->ms += t; r->flops += ev.flops;
    }
    size_t pos = 0;
    auto put = [&](const char* fmt, auto... a) {
        if (pos + 1 >= capacity) return;
        int w = snprintf(out + pos, capacity - pos, fmt, a...);
        if (w > 0) pos += (size_t)w < capacity - pos ? (size_t)w : capacity - pos - 1;
    };
    // cus: the launch's workgroup cap under the forward's CU partition (256 = the whole chip); TF/CU-share: TFLOP/s scaled to a whole chip of such CUs
    put("%7s %6s %6s %6s %5s %4s %6s %9s %9s %8s %11s\n", "M", "N", "K", "flags", "tile", "cus", "n", "avg_us", "total_ms", "TFLOP/s", "TF/CU-share");
    for (const auto& r : rows) {
        const int cus = r.cus > 0 && r.cus < 256 ? r.cus : 256;
        const double tf = r.flops / (r.ms * 1e-3) * 1e-12;
        put("%7d %6d %6d %6d %5d %4d %6d %9.2f %9.3f %8.1f %11.1f\n", r.M, r.N, r.K, r.flags, r.tile, cus, r.n, 1e3 * r.ms / r.n, r.ms, tf, tf * 256.0 / cus);
    }
    out[pos < capacity ? pos : capacity - 1] = 0;
    return 0;
}

// ================================================================================================ one-tower handles: what mmhip_txt_* and mmhip_img_* share
// Every entry point of a kind refuses a handle of another kind before it touches it; the accessors forward to the late-fusion ones.
using Kind = mmhip_engine::Kind;
static bool is_kind(mmhip_handle h, Kind k) { return h && h->kind == k; }
// the configuration fields both kinds have
static bool tower_config_ok(int hidden, int heads, int inter, int layers, int dtype, int max_posts, int num_labels, float loss_scale) {
    if (hidden <= 0 || hidden % 128 || hidden > 1024 || heads * 64 != hidden || inter <= 0 || inter % 128 || layers < 0) return false;
    if (max_posts < 1 || max_posts > 1024) return false;
    if (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_BF16X3) return false;
    return num_labels >= 1 && num_labels <= CLS_HEAD_MAX_C && loss_scale >= 0.f;
}
// one trainable buffer, no frozen one; the image tower's pad rows (i_pad_B) are cleared again for a new workspace
static int one_tower_bind(mmhip_handle h, Kind k, float* params, float* grad, void* workspace, uint64_t workspace_bytes) {
    if (!is_kind(h, k) || !params || !workspace) return MMHIP_E_INVALID;
    if (workspace_bytes < h->ws_need) return MMHIP_E_CAPACITY;
    if (((uintptr_t)params | (uintptr_t)grad | (uintptr_t)workspace) & 255) return MMHIP_E_INVALID;
    h->frozen = nullptr; h->train = params; h->grad = grad; h->ws = (char*)workspace; h->ws_bytes = workspace_bytes;
    h->fwd_done = false;
    h->i_pad_B = 0;
    return 0;
}
// opens a forward of B posts (no ITM rows): nothing of an earlier forward, loss or backward survives; no CU partition (one tower)
static int one_tower_begin(mmhip_engine& e, int B, int T, int train, uint64_t seed) {
    e.B = e.Bt = B; e.T = T; e.itm = false; e.train_mode = train != 0; e.seed = seed;
    e.fwd_done = false; e.bwd_begun = false; e.bd_out_cls = nullptr; e.bd_logits = e.bd_out_tim = e.bd_feats = nullptr; e.bd_itc_global = false;
    e.cur_part[0] = e.cur_part[1] = 0;
    return side_init(e);
}
static int one_tower_step_guard(mmhip_handle h, Kind k, const float* adam_m, const float* adam_v, const int64_t* onehot, int step) {
    if (!is_kind(h, k) || !h->ws || !h->grad) return MMHIP_E_STATE;
    if (!adam_m || !adam_v || !onehot || step < 1) return MMHIP_E_INVALID;
    return 0;
}

// ================================================================================================ text-only handle (mmhip_txt_*)
// The reference's text-only trainer (models/text_only.py: BERT / BERNICE + TextModel.train): the text tower of this engine -- the same layer launch
// sequences, forward and backward -- under the fused CLS classifier head, without the image tower and the dual-encoder heads.
int mmhip_txt_create(const mmhip_txt_config* cfg, mmhip_txt_handle* out) {
    if (!cfg || !out) return MMHIP_E_INVALID;
    const mmhip_txt_config& t = *cfg;
    if (!tower_config_ok(t.hidden, t.heads, t.inter, t.layers, t.dtype, t.max_posts, t.num_labels, t.loss_scale)) return MMHIP_E_INVALID;
    if (t.max_text_len > 128 || t.max_text_len < 1 || t.vocab < 1 || t.type_vocab < 1 || t.type_vocab > 2) return MMHIP_E_INVALID;
    if (t.txt_kind != MMHIP_TXT_XLMR && t.txt_kind != MMHIP_TXT_BERT) return MMHIP_E_INVALID;
    if (t.txt_kind == MMHIP_TXT_XLMR && t.max_pos < t.max_text_len + t.pad_id + 1) return MMHIP_E_INVALID;
    if (t.txt_kind == MMHIP_TXT_BERT && t.max_pos < t.max_text_len) return MMHIP_E_INVALID;
    if (t.pad_id < 0 || t.pad_id >= t.vocab || !(t.p_hidden >= 0.f) || !(t.p_attn >= 0.f) || !(t.p_head >= 0.f)) return MMHIP_E_INVALID;
    mmhip_engine* e = new (std::nothrow) mmhip_engine();
    if (!e) return MMHIP_E_INVALID;
    mmhip_config& c = e->cfg;
    c = mmhip_config{};
    c.hidden = t.hidden; c.heads = t.heads; c.inter = t.inter; c.layers_txt = t.layers; c.layers_img = 0;
    c.vocab = t.vocab; c.max_pos = t.max_pos; c.type_vocab = t.type_vocab; c.txt_kind = t.txt_kind; c.pad_id = t.pad_id;
    // image-tower and dual-encoder fields: placeholders that only keep the shared struct's geometry helpers (P(), Hv(), Kpp()) defined -- a text-only
    // handle never launches, carves or lays out anything from them (build_layout_txt, the `mm` branches of build_workspace)
    c.ln_eps_txt = c.ln_eps_img = t.ln_eps; c.image = c.patch = 16; c.proj_dim = 1; c.num_labels = t.num_labels; c.fusion = MMHIP_FUSION_CONCAT;
    c.p_hidden = t.p_hidden; c.p_attn = t.p_attn; c.p_head = t.p_head; c.dtype = t.dtype; c.max_posts = t.max_posts; c.max_text_len = t.max_text_len;
    c.loss_scale = t.loss_scale; c.img_kind = MMHIP_IMG_VIT;
    e->kind = mmhip_engine::TEXT;
    e->tm_prefix = "bert_model.";
    read_x3_env(*e);
    build_layout_txt(*e);
    build_workspace(*e);
    *out = e;
    return 0;
}
void mmhip_txt_destroy(mmhip_txt_handle h) { if (is_kind(h, Kind::TEXT)) mmhip_destroy(h); }
int mmhip_txt_param_count(mmhip_txt_handle h) { return is_kind(h, Kind::TEXT) ? mmhip_param_count(h) : MMHIP_E_INVALID; }
int mmhip_txt_param_info_at(mmhip_txt_handle h, int i, mmhip_param_info* out) { return is_kind(h, Kind::TEXT) ? mmhip_param_info_at(h, i, out) : MMHIP_E_INVALID; }
uint64_t mmhip_txt_numel(mmhip_txt_handle h) { return is_kind(h, Kind::TEXT) ? mmhip_buffer_numel(h, 1) : 0; }
uint64_t mmhip_txt_workspace_bytes(mmhip_txt_handle h) { return is_kind(h, Kind::TEXT) ? mmhip_workspace_bytes(h) : 0; }
int mmhip_txt_bind(mmhip_txt_handle h, float* params, float* grad, void* workspace, uint64_t workspace_bytes) {
    return one_tower_bind(h, Kind::TEXT, params, grad, workspace, workspace_bytes);
}
int mmhip_txt_refresh_weights(mmhip_txt_handle h, void* stream) {
    if (!is_kind(h, Kind::TEXT)) return MMHIP_E_INVALID;
    return mmhip_refresh_weights(h, 2, stream);
}
// forward of the tower and the head; onehot != NULL: the head also leaves loss / correct count / d logits (fused step and mmhip_txt_loss)
static int txt_forward_impl(mmhip_txt_handle h, const int64_t* ids, const int64_t* mask, const int64_t* type_ids, int B, int T, int train, uint64_t seed,
                            const int64_t* onehot, const float* class_w, float* logits, float* loss, int* n_correct, void* stream) {
    if (!is_kind(h, Kind::TEXT) || !h->ws) return MMHIP_E_STATE;
    if (!ids || !mask || B < 1 || T < 1) return MMHIP_E_INVALID;
    mmhip_engine& e = *h;
    if (B > e.cfg.max_posts || T > e.cfg.max_text_len) return MMHIP_E_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    CHECK_RC(one_tower_begin(e, B, T, train, seed));
    CHECK_HIP(launch_copy_ids_clamped(ids, e.wsp<int64_t>(e.ids_all), (size_t)B * T, e.cfg.vocab, e.bad_index, s));
    CHECK_HIP(hipMemcpyAsync(e.ws + e.mask_all, mask, (size_t)B * T * 8, hipMemcpyDeviceToDevice, s));
    // a one-row type table has nothing to select: every token takes row 0 whatever the caller passes (RoBERTa-shaped checkpoints)
    e.has_tt = type_ids != nullptr && e.cfg.type_vocab > 1;
    if (e.has_tt) CHECK_HIP(launch_copy_ids_clamped(type_ids, e.wsp<int64_t>(e.tt_all), (size_t)B * T, e.cfg.type_vocab, e.bad_index, s));
    CHECK_RC(e.span(0, s));
    CHECK_RC(text_forward(e, s));
    CHECK_RC(e.span(2, s));
    CHECK_RC(cls_head_forward(e, txt_head_args(e), onehot, class_w, logits, loss, n_correct, s));
    CHECK_RC(e.span(3, s));
    e.fwd_done = true;
    return 0;
}
int mmhip_txt_forward(mmhip_txt_handle h, const int64_t* ids, const int64_t* mask, const int64_t* type_ids, int B, int T, int train, uint64_t seed,
                      float* logits, void* stream) {
    return txt_forward_impl(h, ids, mask, type_ids, B, T, train, seed, nullptr, nullptr, logits, nullptr, nullptr, stream);
}
int mmhip_txt_loss(mmhip_txt_handle h, const int64_t* onehot, const float* class_w, float* loss, int* n_correct, void* stream) {
    if (!is_kind(h, Kind::TEXT) || !h->fwd_done) return MMHIP_E_STATE;
    if (!onehot) return MMHIP_E_INVALID;
    return cls_head_forward(*h, txt_head_args(*h), onehot, class_w, nullptr, loss, n_correct, (hipStream_t)stream);
}
int mmhip_txt_backward(mmhip_txt_handle h, const float* d_logits, void* stream) {
    if (!is_kind(h, Kind::TEXT)) return MMHIP_E_STATE;
    return mmhip_backward(h, d_logits, nullptr, nullptr, nullptr, stream);
}
int mmhip_txt_set_grad_clip(mmhip_txt_handle h, float max_norm, void* clip_state) {
    return is_kind(h, Kind::TEXT) ? mmhip_set_grad_clip(h, max_norm, clip_state) : MMHIP_E_INVALID;
}
int mmhip_txt_train_step(mmhip_txt_handle h, const int64_t* ids, const int64_t* mask, const int64_t* type_ids, const int64_t* onehot, const float* class_w,
                         int B, int T, uint64_t seed, float* adam_m, float* adam_v, float lr, float beta1, float beta2, float eps, float weight_decay,
                         int step, float* loss, int* n_correct, void* stream) {
    CHECK_RC(one_tower_step_guard(h, Kind::TEXT, adam_m, adam_v, onehot, step));
    CHECK_RC(clip_step_check(*h, 0, 0));
    CHECK_RC(txt_forward_impl(h, ids, mask, type_ids, B, T, 1, seed, onehot, class_w, nullptr, loss, n_correct, stream));
    return step_backward_update(h, 0, 0, adam_m, adam_v, lr, beta1, beta2, eps, weight_decay, step, 1.0f, stream, nullptr, nullptr);
}

// ================================================================================================ image-only handle (mmhip_img_*)
// The reference's image-only trainer (models/image_only.py `vit` branch + ImageModel.train): HF ViTForImageClassification as a trainable pre-LN tower.
int mmhip_img_create(const mmhip_img_config* cfg, mmhip_img_handle* out) {
    if (!cfg || !out) return MMHIP_E_INVALID;
    const mmhip_img_config& t = *cfg;
    if (!tower_config_ok(t.hidden, t.heads, t.inter, t.layers, t.dtype, t.max_posts, t.num_labels, t.loss_scale)) return MMHIP_E_INVALID;
    if (t.patch < 2 || t.image < t.patch || t.image % t.patch || (3 * t.patch * t.patch) % 64) return MMHIP_E_INVALID;
    const int P = (t.image / t.patch) * (t.image / t.patch) + 1;
    if (P < 129 || P > 288) return MMHIP_E_INVALID;          // what launch_attn_bwd_long takes (160 px and 384 px are out of scope)
    if (!(t.ln_eps > 0.f)) return MMHIP_E_INVALID;
    if (t.p_hidden != 0.f || t.p_attn != 0.f) return MMHIP_E_INVALID;          // the checkpoints' tower dropouts are 0: no dropout is built into this path
    mmhip_engine* e = new (std::nothrow) mmhip_engine();
    if (!e) return MMHIP_E_INVALID;
    mmhip_config& c = e->cfg;
    c = mmhip_config{};
    c.hidden = t.hidden; c.heads = t.heads; c.inter = t.inter; c.layers_txt = 0; c.layers_img = t.layers;
    // text-tower and dual-encoder fields: placeholders -- an image-only handle never lays out, carves or launches anything from them
    c.vocab = 1; c.max_pos = 1; c.type_vocab = 1; c.txt_kind = MMHIP_TXT_BERT; c.pad_id = 0; c.max_text_len = 1; c.proj_dim = 1; c.fusion = MMHIP_FUSION_CONCAT;
    c.ln_eps_txt = c.ln_eps_img = t.ln_eps; c.image = t.image; c.patch = t.patch; c.num_labels = t.num_labels; c.dtype = t.dtype; c.max_posts = t.max_posts;
    c.loss_scale = t.loss_scale; c.img_kind = MMHIP_IMG_VIT;
    e->kind = mmhip_engine::IMAGE;
    read_x3_env(*e);
    build_layout_img(*e);
    build_workspace_img(*e);
    *out = e;
    return 0;
}
void mmhip_img_destroy(mmhip_img_handle h) { if (is_kind(h, Kind::IMAGE)) mmhip_destroy(h); }
int mmhip_img_param_count(mmhip_img_handle h) { return is_kind(h, Kind::IMAGE) ? mmhip_param_count(h) : MMHIP_E_INVALID; }
int mmhip_img_param_info_at(mmhip_img_handle h, int i, mmhip_param_info* out) { return is_kind(h, Kind::IMAGE) ? mmhip_param_info_at(h, i, out) : MMHIP_E_INVALID; }
uint64_t mmhip_img_numel(mmhip_img_handle h) { return is_kind(h, Kind::IMAGE) ? mmhip_buffer_numel(h, 1) : 0; }
uint64_t mmhip_img_workspace_bytes(mmhip_img_handle h) { return is_kind(h, Kind::IMAGE) ? mmhip_workspace_bytes(h) : 0; }
int mmhip_img_bind(mmhip_img_handle h, float* params, float* grad, void* workspace, uint64_t workspace_bytes) {
    return one_tower_bind(h, Kind::IMAGE, params, grad, workspace, workspace_bytes);
}
int mmhip_img_refresh_weights(mmhip_img_handle h, void* stream) {
    if (!is_kind(h, Kind::IMAGE)) return MMHIP_E_INVALID;
    if (!h->ws) return MMHIP_E_STATE;
    return img_refresh(*h, (hipStream_t)stream);
}
static int img_forward_impl(mmhip_img_handle h, const float* pixels, int B, int train, const int64_t* onehot, const float* class_w, float* logits, float* loss,
                            int* n_correct, void* stream) {
    if (!is_kind(h, Kind::IMAGE) || !h->ws) return MMHIP_E_STATE;
    if (!pixels || B < 1) return MMHIP_E_INVALID;
    mmhip_engine& e = *h;
    if (B > e.cfg.max_posts) return MMHIP_E_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    CHECK_RC(one_tower_begin(e, B, 1, train, 0));
    CHECK_RC(e.span(0, s));
    if (e.i_pad_B != B) CHECK_RC(img_zero_pads(e, B, s));
    CHECK_RC(image_layers_forward(e, pixels, true, s));
    CHECK_RC(e.span(1, s));
    CHECK_RC(img_head_forward(e, onehot, class_w, logits, loss, n_correct, s));
    CHECK_RC(e.span(3, s));
    e.fwd_done = true;
    return 0;
}
int mmhip_img_forward(mmhip_img_handle h, const float* pixels, int B, int train, float* logits, void* stream) {
    return img_forward_impl(h, pixels, B, train, nullptr, nullptr, logits, nullptr, nullptr, stream);
}
int mmhip_img_loss(mmhip_img_handle h, const int64_t* onehot, const float* class_w, float* loss, int* n_correct, void* stream) {
    if (!is_kind(h, Kind::IMAGE) || !h->fwd_done) return MMHIP_E_STATE;
    if (!onehot) return MMHIP_E_INVALID;
    return cls_head_forward(*h, img_head_args(*h), onehot, class_w, nullptr, loss, n_correct, (hipStream_t)stream);
}
int mmhip_img_backward(mmhip_img_handle h, const float* d_logits, void* stream) {
    if (!is_kind(h, Kind::IMAGE)) return MMHIP_E_STATE;
    return mmhip_backward(h, d_logits, nullptr, nullptr, nullptr, stream);
}
int mmhip_img_set_grad_clip(mmhip_img_handle h, float max_norm, void* clip_state) {
    return is_kind(h, Kind::IMAGE) ? mmhip_set_grad_clip(h, max_norm, clip_state) : MMHIP_E_INVALID;
}
int mmhip_img_train_step(mmhip_img_handle h, const float* pixels, const int64_t* onehot, const float* class_w, int B, float* adam_m, float* adam_v,
                         float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* loss, int* n_correct, void* stream) {
    CHECK_RC(one_tower_step_guard(h, Kind::IMAGE, adam_m, adam_v, onehot, step));
    CHECK_RC(clip_step_check(*h, 0, 0));
    CHECK_RC(img_forward_impl(h, pixels, B, 1, onehot, class_w, nullptr, loss, n_correct, stream));
    return step_backward_update(h, 0, 0, adam_m, adam_v, lr, beta1, beta2, eps, weight_decay, step, 1.0f, stream, nullptr, nullptr);
}

}  // extern "C"
