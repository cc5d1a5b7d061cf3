/* pathomic_hip.h - C-ABI of libpathomic_hip.so (MI355X / gfx950).
 *
 * The reference (CityU-AIM-Group/MultiModal-learning) has no FFI layer: its hot path is pure Python on
 * torch built-ins.  This header is therefore the boundary a maintainer binds
 * (ctypes stub in INTEGRATION.md) to replace the torch ops under the reference's Python module API;
 * each entry cites the reference site (path relative to /root/reference/MICCAI-2022) it replaces.
 *
 * Conventions: plain pointers to DEVICE memory + sizes, no torch types; every call enqueues work on
 * `stream` and returns immediately; return 0 on success, negative errno-style code otherwise
 * (-22 invalid argument, -5 launch failure, -16 busy).  No device memory is allocated inside: callers pass workspaces.
 * Thread-compatible (one stream per call).  Process-wide state the library owns: per device ONE side stream and a pool of
 * 16 x 64 events for the two-stream trunk backward (created by the first ph_resnet_backward* call outside a stream capture,
 * never destroyed; a 17th backward in flight at once gets -16), the records of the in-library kernel timer (ph_prof_*), and
 * per-kernel "attributes set" flags.  A plan (PhResnetPlan) additionally remembers, per workspace, the pre-packed input of
 * the last forward that ran on it.
 */
#ifndef PATHOMIC_HIP_H_
#define PATHOMIC_HIP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* ph_stream_t; /* a hipStream_t */

#define PH_PREC_BF16 0   /* perf mode: bf16 operands + activations, fp32 accumulate/statistics */
#define PH_PREC_BF16X6 1 /* parity mode: fp32 activations, 3-plane split-bf16 (6-product, fp32-equivalent) MFMA */
#define PH_PREC_BF16X3 2 /* fp32 activations, the 3 leading split-bf16 products (16-bit operands): half the matrix work */
#define PH_PREC_FP16X3 3 /* half-pair mode: tensors a convolution reads are fp16 pairs x = hi + lo * 2^-11 (4 B / element, 22
                            significant bits), conv outputs / gradients fp32, 3 fp16 MFMA products (hi*hi, hi*lo, lo*hi) */

#define PH_PREC_FP16X1 4 /* only as the backward arithmetic of a PH_PREC_FP16X3 plan (set_backward_prec below): dgrad / wgrad on the hi planes alone */

#define PH_ACT_NONE 0
#define PH_ACT_RELU 1
#define PH_ACT_ELU 2
#define PH_ACT_SIGMOID 3

#define PH_EW_RELU 0
#define PH_EW_GATE 1
#define PH_EW_RELU_BWD 2
#define PH_EW_ADD 3
#define PH_EW_ELU_BWD 4  /* a * ELU'(x) given b = ELU(x) */
#define PH_EW_MUL 5

int ph_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * BasicBlock ResNet trunk: conv7x7/2-BN-ReLU-maxpool, four layers of layers4[0..3] BasicBlocks at 64 / 128 / 256 / 512
 * channels (ResNet-18: {2, 2, 2, 2}, ResNet-34: {3, 4, 6, 3}), global avg-pool of layer3 and layer4.
 * Replaces ResNet._forward_impl up to the pooled features (resnets.py:217-236, BasicBlock :58-74) and
 * its autograd backward.  Train-mode BatchNorm everywhere (train_test_path_multi_distill.py:231-232).
 *
 * A "unit" is one convolution with its BatchNorm.  Units follow state_dict order: conv1/bn1, then per block conv1/bn1,
 * conv2/bn2, downsample.0/downsample.1 (block 0 of layers 2-4 only).  A plan has
 * N (ph_resnet_num_units) = 1 + 2 * (layers4[0] + .. + layers4[3]) + 3 of them: 20 for ResNet-18, 36 for ResNet-34.
 * Blocks are numbered 0 .. sum(layers4) - 1 in the same order.
 *
 * params: N units x 6 pointers [conv weight OIHW f32, bn weight, bn bias, running_mean, running_var,
 *         num_batches_tracked (int64)].
 * grads : N units x 3 pointers [d conv weight (OIHW f32), d bn weight, d bn bias] (overwritten).
 *
 * ph_resnet_plan_create_layers returns NULL, before any allocation or HIP call, for layers4 == NULL, an entry below 1 or
 * above PH_RESNET_MAX_BLOCKS, B < 1, H or W < 32, an unknown prec, or PH_PREC_FP16X3 with H or W no multiple of 4.
 * ph_resnet_plan_create is ph_resnet_plan_create_layers with layers4 = {2, 2, 2, 2}.
 * ---------------------------------------------------------------------------------------------- */
#define PH_RESNET_MAX_BLOCKS 64  /* BasicBlocks per layer (torchvision's deepest stage, ResNet-152 layer3, has 36) */
typedef struct PhResnetPlan PhResnetPlan;
PhResnetPlan* ph_resnet_plan_create(int B, int H, int W, int prec);
PhResnetPlan* ph_resnet_plan_create_layers(int B, int H, int W, int prec, const int* layers4);
void ph_resnet_plan_destroy(PhResnetPlan* plan);
size_t ph_resnet_workspace_bytes(const PhResnetPlan* plan);
size_t ph_resnet_packed_bytes(const PhResnetPlan* plan);
int ph_resnet_num_units(const PhResnetPlan* plan);
int ph_resnet_unit_shape(const PhResnetPlan* plan, int unit, int* out4 /* Cout, Cin, KS, stride */);
/* OIHW fp32 -> MFMA operand layouts (bf16 hi/lo planes, fwd [tap][O][I] and dgrad [tap][I][O]); call after
 * every optimiser step */
int ph_resnet_pack_weights(const PhResnetPlan* plan, const void* const* params, void* packed, ph_stream_t stream);
/* Signature of the packed-weight layout `plan` reads under the current kernel switches (half-pair mode: which units' weights are
 * fragment-major).  A packed buffer is valid for every plan of the same precision whose signature equals the one of the plan
 * that packed it; re-pack when it differs.  The call refreshes the plan's layout to the current switches. */
unsigned long long ph_resnet_plan_layout_sig(const PhResnetPlan* plan);
/* x_nchw [B,3,H,W] f32 -> f3 [B,256], f4 [B,512] f32 (either may be NULL).  flags bit0: train mode, update the running
 * statistics; bit1: eval mode (normalise with the running statistics; no backward); bit2: forward only - no
 * ph_resnet_backward will read this workspace (the no_grad EMA / teacher forwards of train_test_path_multi_distill.py:
 * 253-256): bn1 + ReLU of every BasicBlock (resnets.py:61-63) is then applied by conv2 while it stages its input and the
 * a1 tensor is not materialised (perf mode); bit3: keep the separate passes nevertheless (A/B and test switch); bit4 /
 * bit5: A/B and test switches (first-generation stride-2 kernel / separate stem conv and pooling passes); bit6: `x_nchw`
 * is the NHWC4 tensor ph_pack_input made of the image (the student and the teacher read the same x_path,
 * train_test_path_multi_distill.py:249,256: packed once) - it must stay valid until the matching backward has run */
/* Arithmetic of the backward's dgrad / wgrad launches where it differs from the plan's (PH_PREC_BF16X3 on a PH_PREC_BF16X6
 * plan: parity-mode forward, three-product backward; PH_PREC_FP16X1 on a PH_PREC_FP16X3 plan: three-product forward, the hi
 * planes' product alone in the backward; -1 = follow the plan) */
int ph_resnet_plan_set_backward_prec(const PhResnetPlan* plan, int prec);
/* Scheduling of ph_resnet_backward / _part: 1 (default) = the weight-gradient launches run on a second, process-wide
 * stream of the library (created once per device, never destroyed) beside the BatchNorm-backward / dgrad chain and are
 * joined before the call returns (inside a stream capture: a parallel branch of the graph); 0 = everything on the
 * caller's stream.  Same kernels; BatchNorm gradients bitwise the same,
 * weight gradients summed from half as many partial slabs (autograd of resnets.py:58-74 has no order between a layer's
 * weight and input gradients either). */
int ph_resnet_plan_set_backward_overlap(const PhResnetPlan* plan, int on);
/* The stem's backward in the bf16 mode of ph_resnet_backward / _part: 1 (default; the environment variable PH_STEM_FUSE=0/1 sets
 * the value a new plan starts with) = the stem's weight-gradient kernel forms the gradient at the stem conv's output itself,
 * from the conv output, the pooled gradient and the arg codes - that 64-channel tensor is neither written nor read; 0 = a pass
 * of its own writes it first.  Bitwise the same gradients.  The other arithmetics, ph_resnet_backward_input and a cut debug
 * backward always run the separate pass. */
int ph_resnet_plan_set_stem_fused(const PhResnetPlan* plan, int on);
int ph_pack_input(const float* x_nchw, void* x4 /* B*H*W*4 elements of the mode's activation type */, int B, int H, int W,
                  int prec, ph_stream_t stream);
int ph_resnet_forward(const PhResnetPlan* plan, const void* const* params, const void* packed, const float* x_nchw,
                      void* workspace, float* f3, float* f4, int flags, ph_stream_t stream);
int ph_resnet_backward(const PhResnetPlan* plan, const void* const* params, const void* packed, void* workspace,
                       const float* g_f3 /* may be NULL */, const float* g_f4, void* const* grads,
                       ph_stream_t stream);
/* The same backward in two calls for a data-parallel caller: part 0 = every block of layers 4 and 3 (afterwards the
 * gradients of layers 3-4, 93 % of the trunk's parameter bytes, are final and their all-reduce can start), part 1 = layers
 * 2, 1 and the stem; part -1 = everything (== ph_resnet_backward).  The reference's DataParallel reduces after the whole
 * backward (utils.py:257-260). */
int ph_resnet_backward_part(const PhResnetPlan* plan, const void* const* params, const void* packed, void* workspace,
                            const float* g_f3, const float* g_f4, void* const* grads, int part, ph_stream_t stream);
/* Test access: the same backward cut off after `stop_after` >= 1 launch groups ("stages": the avgpool backward, then per
 * BasicBlock bn2 / wgrad(conv2) / dgrad(conv2) / bn1 / wgrad(conv1) / dgrad(conv1) [+ bn / wgrad / dgrad of the
 * downsample branch], then the stem's BatchNorm reduction, its apply pass, its weight gradient) - autograd of
 * resnets.py:58-74,219-222 one node at a time.  Only scratch buffers are written, so it can be re-run; with
 * the tensor-info call below - its `what` 4-9 are the scratch buffers, the BatchNorm statistics and the pool arg codes - a harness compares
 * every stage with a reference computed from that stage's own inputs (tests/test_gpu_fullsize.py). */
int ph_resnet_backward_debug(const PhResnetPlan* plan, const void* const* params, const void* packed, void* workspace,
                             const float* g_f3, const float* g_f4, void* const* grads, int stop_after, ph_stream_t stream);
/* Gradient with respect to the image [B,3,H,W] f32 of an EVAL-mode forward (flags bit1; BatchNorm backward is then
 * gamma * invstd * dz, no parameter gradients).  The reference needs it for the MIA-2023 stage-1 superpixel attention
 * masks ("MIA 2023/stage1_multi_modal_teacher/train_test_MT_SP_Masking.py":62-75: model.eval(); cost.backward();
 * x_path.grad).  ph_stem_dgrad is its last step (input gradient of the 7x7/2 conv; dy NHWC of the mode's type). */
int ph_resnet_backward_input(const PhResnetPlan* plan, const void* const* params, const void* packed, void* workspace,
                             const float* g_f3 /* may be NULL */, const float* g_f4, float* dx_nchw, ph_stream_t stream);
int ph_stem_dgrad(const void* dy_nhwc, const float* w_oihw, float* dx_nchw, int B, int H, int W, int prec,
                  ph_stream_t stream);
int ph_resnet_tensor_info(const PhResnetPlan* plan, int what, int id, size_t* byte_off, int* dims4);

/* ------------------------------------------------------------------------------------------------
 * Dense fp32 operators of the heads / SNN / fusion (resnets.py:165-169,239-250; networks_new.py:185-251;
 * fusion.py:36-63).  C[m][n] = act(sum_k A[m*sam+k*sak] * B[k*sbk+n*sbn] + bias[n]) (+C)
 * ph_sgemm_splitk sums K in at most nsplit slabs of a multiple of 32 (fewer where K / 32 is smaller); nsplit < 1 returns
 * PH_EINVAL before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
int ph_sgemm(const float* A, const float* B, const float* bias, float* C, int M, int N, int K, long sam, long sak,
             long sbk, long sbn, long ldc, int act, int accumulate, ph_stream_t stream);
int ph_sgemm_splitk(const float* A, const float* B, const float* bias, float* C, float* part /* nsplit*M*N */,
                    int nsplit, int M, int N, int K, long sam, long sak, long sbk, long sbn, long ldc, int act,
                    ph_stream_t stream);
/* nn.BatchNorm1d training mode (+ReLU) and backward (resnets.py:165-167; fusion.py:29-32) */
int ph_bn1d_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* invstd,
                float* running_mean, float* running_var, int64_t* num_batches_tracked, int B, int C, float eps,
                float momentum, int relu, ph_stream_t stream);
/* eval mode (module.eval(): running statistics), used by the reference's test() (train_test_path_multi_distill.py:409-411) */
int ph_bn1d_eval(const float* x, const float* gamma, const float* beta, const float* running_mean,
                 const float* running_var, float* y, int B, int C, float eps, int relu, ph_stream_t stream);
/* backward of the eval-mode form (a fixed per-channel scale): needed when a gradient flows THROUGH an eval-mode net to its
 * input (train_test_MT_SP_Masking.py:62-75) */
int ph_bn1d_eval_bwd(const float* g, const float* y, const float* gamma, const float* running_var, float* dx, int B, int C,
                     float eps, int relu, ph_stream_t stream);
int ph_bn1d_bwd(const float* g, const float* y, const float* x, const float* mean, const float* invstd,
                const float* gamma, float* dx, float* dgamma, float* dbeta, int B, int C, int relu,
                ph_stream_t stream);
/* nn.LogSoftmax(dim=1) (networks_new.py:139-140), F.nll_loss mean (train_test_path_multi_distill.py:262) */
int ph_log_softmax(const float* x, float* y, int B, int C, ph_stream_t stream);
int ph_log_softmax_bwd(const float* g, const float* y, float* dx, int B, int C, ph_stream_t stream);
int ph_nll_fwd(const float* pred, const int64_t* grade, float* loss, int B, int C, float inv_bnorm,
               ph_stream_t stream);
int ph_nll_bwd(const float* gscalar, const int64_t* grade, float* dpred, int B, int C, float inv_bnorm,
               ph_stream_t stream);
/* DistillKL.forward / backward w.r.t. y_s (KD_loss.py:13-17) */
int ph_kl_fwd(const float* y_s, const float* y_t, float* loss, int B, int C, float T, float inv_bnorm,
              ph_stream_t stream);
int ph_kl_bwd(const float* gscalar, const float* y_s, const float* y_t, float* dy_s, int B, int C, float T,
              float inv_bnorm, ph_stream_t stream);
/* MIA-2023 per-sample DistillKL ("MIA 2023/stage2_unimodal_student/KD_loss.py":14-20) and its backward */
int ph_kl_rows_fwd(const float* y_s, const float* y_t, float* sample_loss, int B, int C, float T, ph_stream_t stream);
int ph_kl_rows_bwd(const float* g_rows, const float* y_s, const float* y_t, float* dy_s, int B, int C, float T,
                   ph_stream_t stream);
/* assign_sample_weights ("MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":131-158), from logits */
int ph_conf_discrepancy(const float* logit_s, const float* logit_t, const int64_t* gt, float* out, int B, int C,
                        float max_discrep, ph_stream_t stream);
/* Normalize(2) of Embed (CL_utils/CRD_loss.py:263-267,276-279) */
int ph_l2norm_fwd(const float* x, float* y, float* norm, int B, int D, ph_stream_t stream);
int ph_l2norm_bwd(const float* g, const float* y, const float* norm, float* dx, int B, int D, ph_stream_t stream);
int ph_eltwise(const float* a, const float* b, float* out, size_t n, int op, ph_stream_t stream);
/* o1 (x) o2 with optional appended ones (fusion.py:56-58) / nn.Bilinear operand (fusion.py:43,50) */
int ph_outer(const float* o1, const float* o2, float* o12, int B, int D1, int D2, int append_one,
             ph_stream_t stream);
/* nn.Dropout / nn.AlphaDropout, training mode, counter-based RNG (fusion.py:22-32; networks_new.py:193) */
int ph_dropout(float* x, size_t n, float p, uint64_t seed, uint64_t offset, int alpha, ph_stream_t stream);
/* HIP-graph-replayable form: the per-step part of the counter is read from device memory */
int ph_dropout_dev(float* x, size_t n, float p, uint64_t seed, uint64_t site_offset, const uint64_t* step_counter,
                   int alpha, ph_stream_t stream);
int ph_counter_inc(uint64_t* counter, ph_stream_t stream);
/* Backward of the SNN / fusion operators (stage-1 teacher training, SURVEY row f-1: train_test_MT.py:42-337 needs the
 * gradients of networks_new.py:223-251 and fusion.py:36-63).  ph_dropout_bwd_dev re-creates the forward mask from the
 * same (seed, site_offset, step counter value); ph_gate_bwd: y = sigmoid(z) * h; ph_outer_bwd: the two operands of
 * ph_outer. */
int ph_dropout_bwd_dev(float* g, size_t n, float p, uint64_t seed, uint64_t site_offset, const uint64_t* step_counter,
                       int alpha, ph_stream_t stream);
/* the same two out of place (dst = f(src); src == dst allowed): one launch per dropout site instead of a copy + an in-place
 * launch on the latency-bound head chains of the step */
int ph_dropout_dev_to(const float* src, float* dst, size_t n, float p, uint64_t seed, uint64_t site_offset,
                      const uint64_t* step_counter, int alpha, ph_stream_t stream);
int ph_dropout_bwd_dev_to(const float* src, float* dst, size_t n, float p, uint64_t seed, uint64_t site_offset,
                          const uint64_t* step_counter, int alpha, ph_stream_t stream);
int ph_gate_bwd(const float* g, const float* z, const float* h, float* dz, float* dh, size_t n, ph_stream_t stream);
int ph_outer_bwd(const float* g, const float* o1, const float* o2, float* do1, float* do2, int B, int D1, int D2,
                 int append_one, ph_stream_t stream);
int ph_sum(const float* x, float* out, int n, float scale, ph_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * CRD memory bank (DC-Distill): ContrastMemory_v3.forward (CL_utils/memory_new.py:249-397) and
 * ContrastLoss_v2 (CL_utils/CRD_loss.py:221-244).  v1 = student embedding, v2 = teacher embedding,
 * mem1/mem2 = memory_v1/memory_v2 [n_data][feat_dim] f32, feat_dim (the row width) one of 64, 128, 256; params = the module's `params` buffer
 * [K, T, Z_v1, Z_v2, momentum, P].
 * ---------------------------------------------------------------------------------------------- */
/* Sizes are checked on the host before anything is launched; PH_EINVAL for: ph_crd_score B < 1 or PK < 1; ph_crd_select B < 1,
 * P < 1, K < 0, P2 < 1, K2 < 0, P2 > P, K2 > K, an unranked side that does not keep every column (P2 != P / K2 != K) or a ranked
 * list above 160 KiB of LDS ((2 P + K) * 4 bytes); ph_crd_zsum n < 1; ph_crd_update B < 1; ph_crd_loss_grad B < 1, P2 < 1, K2 < 0
 * or P2 + K2 > PK (ph_crd_loss_grad_pos: B < 1, P < 1, m_neg < 1); feat_dim outside {64, 128, 256} everywhere, before any launch. */
/* idx_bank2: optional second index array for memory_v2 (MIA-2023 v10: each bank has its own KNN positives); NULL = idx */
int ph_crd_score(const float* v1, const float* v2, const int64_t* idx /* [B][P+K] */, const int64_t* idx_bank2,
                 const float* mem1, const float* mem2, float* out1, float* out2, float* diff /* each [B][P+K] */,
                 int B, int PK, int feat_dim, float T, ph_stream_t stream);
/* ranks: the P2 host-RNG ranks of memory_new.py:311 (int32, device) or NULL for "hard" (:308) */
int ph_crd_select(const float* diff, const float* out1, const float* out2, const int* ranks, int* sel /* [B][P2+K2] */,
                  float* xs, float* xt /* gathered raw scores [B][P2+K2] */, int B, int P, int K, int P2, int K2,
                  int select_neg, int select_pos /* 0: keep every positive column in order (v3 / v10 banks) */,
                  ph_stream_t stream);
/* DSCD selection of the MIA-2022 tree ("MIA 2022/CL_utils/memory_new.py": ContrastMemory_v4 :471-527, ContrastMemory_mono
 * :630-670): the P positives ranked by diff - ascending = 1 (v4: t_relation - s_relation descending with mem1 the student bank)
 * or 0 (mono: mem1 the teacher bank), the lower column first among equal keys, -0 == +0 - P2 of them at `ranks` (NULL: the first
 * P2 ranks), slot 0 forced to column 0, then ALL K negatives in order: sel / xs / xt are [B][P2 + K].  neg_reweight = 1 (v4
 * :510-517): xs / xt of negative column P + k are out * (1.0f + diff), one rounded add then one rounded multiply, in both
 * directions.  LDS holds the positives alone (2 P words).  PH_EINVAL before any launch for a NULL pointer (ranks excepted), B < 1,
 * P < 1, K < 1, P2 outside 1..P, a flag outside {0, 1} or a positive list above 160 KiB of LDS (P > 20480). */
int ph_crd_select_dscd(const float* diff, const float* out1, const float* out2, const int* ranks, int* sel /* [B][P2+K] */,
                       float* xs, float* xt /* [B][P2+K] */, int B, int P, int K, int P2, int ascending, int neg_reweight,
                       ph_stream_t stream);
int ph_crd_zsum(const float* xs, const float* xt, float* sums2, int n, ph_stream_t stream);
int ph_crd_setz(float* params, const float* sums2, float count, float n_data, ph_stream_t stream);
/* loss partials lossp[B] (sum = s_loss + t_loss) and d loss/d v1, d loss/d v2 [B][feat_dim] */
/* posw_s / posw_t: optional per-positive weights [B][P2] (MIA-2023 ContrastLoss_v2: similarity / sum similarity,
 * "MIA 2023/stage2_unimodal_student/CL_utils/CRD_criterion_v10.py":281-314); NULL = 1/P2 */
int ph_crd_loss_grad(const float* xs, const float* xt, const int* sel, const int64_t* idx, const int64_t* idx_bank2,
                     const float* posw_s, const float* posw_t, const float* mem1, const float* mem2,
                     const float* params, float* lossp, float* dv1, float* dv2, int B, int PK, int P2, int K2,
                     int feat_dim, float n_data, float inv_bnorm, void* workspace /* may be NULL */, ph_stream_t stream);
/* The one-directional half of ph_crd_loss_grad, for ContrastMemory_mono / CRDLoss_v2 ("MIA 2022/CL_utils/memory_new.py":565-698,
 * "MIA 2022/CL_utils/CRD_loss_v2.py":95-101): xt / mem (= memory_v1) / Z_v2 -> lossp [B] and dv = d loss / d v2 [B][feat_dim], bit
 * for bit the dv2 of ph_crd_loss_grad on the same xt, sel, idx, mem and Z_v2, in the one-workgroup and the split form (same
 * workspace size).  params = that bank's [P, K, T, Z_v2, momentum]: only params[3] is read, T is the argument.  posw: optional
 * [B][P2] weights of the positives.  PH_EINVAL for a NULL pointer (posw and workspace excepted), T <= 0 and what ph_crd_loss_grad
 * refuses. */
int ph_crd_loss_grad_one(const float* xt, const int* sel, const int64_t* idx, const float* posw, const float* mem,
                         const float* params, float T, float* lossp, float* dv, int B, int PK, int P2, int K2, int feat_dim,
                         float n_data, float inv_bnorm, void* workspace /* may be NULL */, ph_stream_t stream);
size_t ph_crd_loss_grad_workspace_bytes(int B);                        /* the size at feat_dim 128 */
size_t ph_crd_loss_grad_workspace_bytes_w(int B, int feat_dim);        /* the size at any supported width */
/* Bank-scan form of the CRD negatives: BASELINE configs[4] read as nce_k = 65536 negatives per query (SURVEY 8-e assumption (i);
 * the reference gathers them: "MIA 2023/stage2_unimodal_student/CL_utils/CRD_criterion_v10.py":68-70,106-107,140-141 index_select +
 * bmm over [B][K+1][128], and sums their terms in ContrastLoss_v2 :300-306).  With K at or above the number of bank rows the same
 * sums are taken over ALL rows weighted by multiplicity:
 *   ph_crd_neg_hist:  mult[b][r] = #{k : idx[b * row_stride + col0 + k] == r}, k < K  (mult [B][n_data] int32, every element written);
 *   scores S1 = v1 . bank2^T, S2 = v2 . bank1^T ([B][n_data], ph_sgemm);
 *   ph_crd_scan_neg with zsum_only = 1 (first call of a bank: zsums[0..1] += sum mult exp(S / T), the negatives' share of :146-153's means)
 *   ph_crd_scan_neg with zsum_only = 0: loss_neg[b] = -inv_bnorm sum_r mult (log(m Pn / (x1 + c)) + log(m Pn / (x2 + c))), x = exp(S / T) / Z,
 *     and S1, S2 overwritten by d loss / d S = inv_bnorm mult (x / (x + c)) / T, so that dv1 += S1 . bank2, dv2 += S2 . bank1 (ph_sgemm_splitk);
 *   ph_crd_loss_grad_pos: ph_crd_loss_grad over the P positive columns alone with the NCE constant m Pn of m_neg negatives.
 * params = the memory module's [K T Z_v1 Z_v2 momentum]; loss_neg [B]; zsums [2]. */
int ph_crd_neg_hist(const int64_t* idx, long row_stride, int col0, int K, int B, int n_data, int* mult, ph_stream_t stream);
size_t ph_crd_scan_neg_workspace_bytes(int B, int n_data);
int ph_crd_scan_neg(float* S1, float* S2, const int* mult, const float* params, void* workspace, float* loss_neg, float* zsums,
                    int B, int n_data, int m_neg, float inv_bnorm, int zsum_only, ph_stream_t stream);
int ph_crd_loss_grad_pos(const float* xs, const float* xt, const int* sel, const int64_t* idx, const int64_t* idx_bank2,
                         const float* posw_s, const float* posw_t, const float* mem1, const float* mem2, const float* params,
                         float* lossp, float* dv1, float* dv2, int B, int P, int m_neg, int feat_dim, float n_data, float inv_bnorm,
                         ph_stream_t stream);
/* MIA-2023 v10 KNN positives (CRD_criterion_v10.py:72-79,110-116): class-masked full-bank cosine top-num_pos of each
 * query's own bank row, for both banks; labels = class of every bank row (int32 [n_data]).  1 <= num_pos <= 64 (anything else
 * is PH_EINVAL): nb / sim [B][num_pos] are the rows and similarities of a stable descending sort (lower row first among equal
 * values, -0 = +0); a bank of fewer than num_pos rows leaves the tail at row 0x7fffffff, similarity -inf.  num_pos > 8 runs
 * ceil(num_pos / 8) rank windows (2 + 2 ceil(num_pos / 8) launches per 64 queries, no host read, no allocation).  The workspace
 * size does not depend on feat_dim (a pass takes up to 64 queries at every width, through the same buffers):
 * ph_crd_bank_topk_workspace_bytes is enough for num_pos <= 8, ph_crd_bank_topk_workspace_bytes_np for the num_pos it is given
 * (the same value for num_pos <= 8; 0 for a num_pos outside 1 .. 64).
 * WARNING: the entry cannot see the size of `workspace`.  A call with num_pos > 8 over a buffer sized by
 * ph_crd_bank_topk_workspace_bytes writes up to 2 x 64 x 15 x 8 bytes past its end, with no error: size every workspace by
 * ph_crd_bank_topk_workspace_bytes_np with the num_pos of the call. */
size_t ph_crd_bank_topk_workspace_bytes(int B, int n_data);
size_t ph_crd_bank_topk_workspace_bytes_np(int B, int n_data, int num_pos);
int ph_crd_bank_topk(const float* mem1, const float* mem2, const int* labels, const int64_t* idx, int PK,
                     const int64_t* batch_label, int B, int n_data, int num_pos, int feat_dim, int64_t* nb1,
                     int64_t* nb2, float* sim1, float* sim2, void* workspace, ph_stream_t stream);
int ph_crd_update(float* mem1, float* mem2, const float* v1, const float* v2, const int64_t* y, const float* params,
                  int B, int feat_dim, ph_stream_t stream);
/* ContrastMemory_v3.forward as a STANDALONE call returning (out_v1, out_v2) [B][P2+K2] (memory_new.py:362-379: selected
 * scores / Z); also gathers the selected PRE-update bank rows (rows1 from memory_v1, rows2 from memory_v2, each
 * [B][P2+K2][feat_dim]) that its backward needs after the in-call momentum update (:382-395) has overwritten the bank. */
int ph_crd_outputs(const float* xs, const float* xt, const int* sel, const int64_t* idx, const int64_t* idx_bank2,
                   const float* mem1, const float* mem2, const float* params, float* out1, float* out2, float* rows1,
                   float* rows2, int B, int PK, int S2, int feat_dim, ph_stream_t stream);
/* backward of the above: dv1 = sum_j g1 out1 / T rows2, dv2 = sum_j g2 out2 / T rows1 (g1 / g2 may be NULL = zero) */
int ph_crd_outputs_bwd(const float* g1, const float* g2, const float* out1, const float* out2, const float* rows1,
                       const float* rows2, float T, float* dv1, float* dv2, int B, int S2, int feat_dim,
                       ph_stream_t stream);
/* ContrastLoss_v2.forward (CL_utils/CRD_loss.py:221-252) on x [B][S] with P positives first: rows[b] = the per-sample
 * loss of the sample_KD == "True" branch (:246-250); the "False" branch's scalar (:240-244) is sum(rows) / B.
 * dx[b][j] = d rows[b] / d x[b][j]. */
int ph_contrast_loss_v2(const float* x, float* rows, float* dx, int B, int S, int P, float n_data, ph_stream_t stream);
/* MIA-2023 v10 class-centre positives (`--pos_extra centers --nce_p 2`, CRD_criterion_v10.py:84-89,121-126: the mean
 * bank row of every class, recomputed per call).  mem_ext = a bank allocated with n_data + num_classes rows; row
 * n_data + c receives the mean of rows members[offsets[c] .. offsets[c+1]).  max_class_rows = the largest class. */
size_t ph_crd_class_centers_workspace_bytes(int num_classes, int max_class_rows);                 /* feat_dim 128 */
size_t ph_crd_class_centers_workspace_bytes_w(int num_classes, int max_class_rows, int feat_dim);
int ph_crd_class_centers(float* mem_ext, const int* members, const int* offsets, int num_classes, int max_class_rows,
                         int n_data, int feat_dim, void* workspace, ph_stream_t stream);
/* MIA-2023 v10 clustered class centres (`--pos_extra centers --nce_p N`, N > 2, CRD_criterion_v10.py:81-101,117-137: the
 * reference fits sklearn KMeans(n_clusters = N - 1) on every class of either bank at every call, :90-92 / :126-128).  Here a
 * deterministic Lloyd iteration on the device: farthest-point initialisation from the member at list
 * position 0, `iters` rounds of assignment (least direct-form distance, lowest centre index among equals) and mean update (a
 * centre without members keeps its value).  mem*_ext = banks allocated with n_data + num_classes * k rows; row
 * n_data + c * k + j receives centre j of class c, the n_data bank rows are only read.  Both banks go in every launch;
 * k + 2 * iters launches, no host read, no allocation.  labels (optional) = the last assignment, per bank in list order;
 * counts (optional) = the members of every centre after it.  A class with fewer than k members: centres j >= its size are
 * zero rows without members.  PH_EINVAL for feat_dim != 128, k outside 2 .. 8 (k == 1 is ph_crd_class_centers), iters < 1,
 * num_classes < 1, a NULL or not 16-byte aligned bank, a NULL list or workspace. */
size_t ph_crd_kmeans_centers_workspace_bytes(int num_classes, int max_class_rows, int k);
int ph_crd_kmeans_centers(float* mem1_ext, float* mem2_ext, const int* members, const int* offsets, int num_classes,
                          int max_class_rows, int n_data, int feat_dim, int k, int iters,
                          int* labels /* [2][offsets[num_classes]] or NULL */, int* counts /* [2][num_classes][k] or NULL */,
                          void* workspace, ph_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GK-Refine (AEKD_loss, train_test_path_multi_distill.py:41-70) and optimiser
 * (networks_new.py:85 Adam; train_test_path_multi_distill.py:34-38 update_ema_variables)
 * ---------------------------------------------------------------------------------------------- */
/* Argument rule of the GK-Refine entries, the masks (ph_superpixel_mask, ph_topk_threshold_mask, ph_apply_mask) and the
 * flat-buffer updates and reductions (both Adam forms, ph_adagrad_ema_step_dev, ph_ema_update, ph_ema_update_dev, ph_l1_sum,
 * ph_l1_sign_axpy, ph_sigmoid_range_fwd / _bwd, ph_sqdiff_sum, ph_scaled_diff, ph_maxnorm_mix); all of it is decided on the
 * host before anything is launched:
 *   - a NULL required pointer returns PH_EINVAL.  Optional (may be NULL) are only: ema; losses (with nl == 0) and total of
 *     ph_gk_scale; mo_init (every call is then a first call); e_dev (= 1); mean_out; coef_dev (= 1).
 *   - n == 0 on an elementwise update (both Adam forms, Adagrad, ph_ema_update, ph_ema_update_dev, ph_scaled_diff,
 *     ph_l1_sign_axpy) returns PH_OK and launches nothing.  The reductions: ph_gram needs n >= 1 and ph_maxnorm_mix n >= 1
 *     (PH_EINVAL otherwise: a cosine or a maximum of nothing); ph_sqdiff_sum and ph_l1_sum of n == 0 write 0 (* scale).
 *   - alignment: p, g, m, v and ema of both Adam forms are read and written four floats at a time and must be 16-byte aligned
 *     (train_step.FlatParams places every tensor so); a misaligned one returns PH_EINVAL.  n itself is free: the last 1..3
 *     elements take a scalar path and nothing at or beyond index n is touched.  The other entries need float alignment only.
 * ph_gram: ng in 2..5 (else PH_EINVAL).  ph_gk_scale: ng >= 1, 0 <= nl <= ng.  ph_gk_scale_momentum: ng >= 1. */
int ph_gram(const float* G /* [ng][n] */, float* gram /* [ng*ng] */, int ng, int n, ph_stream_t stream);
int ph_gk_scale(const float* gram, const float* const* losses /* device array of nl device scalars */, int ng, int nl,
                float mult, float* scale, float* total, ph_stream_t stream);
/* Fused forms used by the closed-form loss head of the stage-2 step (multimodal_learning_amd/loss_head.py; reference
 * train_test_path_multi_distill.py:262-313 and AEKD_loss :41-70).  ph_logit_losses: log-softmax, the two DistillKL terms
 * and the NLL of one logit matrix plus d(each loss)/d(logits) for a unit upstream gradient (losses[3], dl[3][B][C]).
 * ph_gk_finish: GK-Refine weights of five gradients in the order [div1, div2, CE, kd1, kd2] from their Gram matrix,
 * w = add + scale * coef, total = w . losses, scaled = losses * logc, scale_ext = scale as [div1, div2, kd1, kd2, CE]. */
int ph_logit_losses(const float* ys, const float* yt1, const float* yt2, const int64_t* grade, float* pred, float* losses,
                    float* dl, int B, int C, float T, float inv_bnorm, ph_stream_t stream);
int ph_gk_finish(const float* gram, const float* losses, const float* coef, const float* add, const float* logc, float mult,
                 float* scale_int, float* w, float* total, float* scaled, float* scale_ext, ph_stream_t stream);
/* momentum_AEKD_loss ("MIA 2022/train_test_path_multi_distill_v2.py":89-132): cosine Gram row sums without the
 * x len(list) factor, optional > thresh binarisation (:114-115), EMA of the weights (:121-124; *mo_init == 0 on the
 * first call, set to 1 by the kernel) */
int ph_gk_scale_momentum(const float* gram, int ng, int use_thresh, float thresh, float momentum, float* mo_scale,
                         int* mo_init, ph_stream_t stream);
/* The closed-form loss head's finish for that trainer (loss_head.py, variant mia2022): gram / losses in the head's internal order
 * [div1, div2, CE, kd1, kd2]; mo_scale (persistent, [5]) and scale_ext in the trainer's order [div1, div2, kd1, kd2, CE];
 * w = gradient weights (lam for CE, mult * state_i * c_i for the distillation terms, c = (alpha, alpha, beta e, beta e) with
 * e = *e_dev, the epoch weight of the CRD terms, :436-437), total = w . losses, scaled = losses * c (:452-455) */
int ph_gk_finish_momentum(const float* gram, const float* losses, float alpha, float beta, const float* e_dev, float lam,
                          float mult, int use_thresh, float thresh, float momentum, float* mo_scale, int* mo_init, float* w,
                          float* total, float* scaled, float* scale_ext, ph_stream_t stream);
/* GK_refine_thresh ("MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":81-128): per-sample cosine
 * matrix of the ng gradients G[ng][B][D] -> all_scale[B][ng]; PH_EINVAL for D outside {64, 128, 256} or ng outside {3, 5} */
int ph_gk_rows(const float* G, int ng, int B, int D, int use_thresh, float thresh, float* all_scale,
               ph_stream_t stream);
int ph_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema /* may be NULL */, size_t n, double lr,
                     double beta1, double beta2, double eps, double weight_decay, int step, double ema_alpha,
                     ph_stream_t stream);
/* HIP-graph-replayable form: hyper = device float[5] {lr, 1-beta1^t, sqrt(1-beta2^t), ema_alpha, 1-ema_alpha}.  beta1 < 0: the
 * betas are read from device memory too, hyper = float[12] with [8..11] = {beta1, 1-beta1, beta2, 1-beta2} (a schedule that
 * cycles beta1 - lr_policy onecycle, networks_new.py:124-125 - reaches a launch replayed from a captured graph) */
int ph_adam_ema_step_dev(float* p, const float* g, float* m, float* v, float* ema /* may be NULL */, size_t n, double beta1,
                         double beta2, double eps, double weight_decay, const float* hyper, ph_stream_t stream);
/* torch.optim.Adagrad as define_optimizer builds it (reference MICCAI-2022/networks_new.py:86-87: lr, weight_decay,
 * initial_accumulator_value = 0.1, lr_decay 0, eps 1e-10): g' = g + wd p, sum += g'^2, p -= lr g' / (sqrt(sum) + eps), with the
 * mean-teacher EMA copy (train_test_path_multi_distill.py:34-38) fused as in ph_adam_ema_step_dev.  hyper: the same device
 * float[5] record ([0] = lr, [3] / [4] = EMA rate and complement). */
int ph_adagrad_ema_step_dev(float* p, const float* g, float* sum, float* ema /* may be NULL */, size_t n, double eps,
                            double weight_decay, const float* hyper, ph_stream_t stream);
int ph_ema_update(float* ema, const float* p, size_t n, float alpha, ph_stream_t stream);
/* define_reg (MICCAI-2022/networks_new.py:93-108 -> utils.py:60-198, the `lambda_reg * loss_reg` term of
 * train_test_MT.py:209-217 and train_test_path_multi_distill.py:312-313): L1 norm of a contiguous run of fp32
 * parameters.  ph_l1_sum: out[0] (+)= sum |w[i]|, `partials` = scratch of >= 1024 floats, fixed summation order.
 * ph_l1_sign_axpy: g[i] += coef * coef_dev[0] * sgn(w[i]) (coef_dev may be NULL = 1), its backward. */
int ph_l1_sum(const float* w, size_t n, float* partials, float* out, int accumulate, ph_stream_t stream);
int ph_l1_sign_axpy(const float* w, float* g, size_t n, const float* coef_dev, float coef, ph_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fine-grained convolution entry points (unit tests / other callers).  Activations NHWC in the precision
 * mode's type, weights OIHW f32.  `ws` must hold ph_conv2d_workspace_bytes().
 * Accepted by all four (fwd, dgrad, dgrad_res, wgrad): KS = 3 with pad 1 at stride 1 or 2, or pad 0 at stride 1; KS = 1 with
 * pad 0 at stride 1 or 2; Cin, Cout multiples of 64; B >= 1 and a non-empty output.  prec: 0..3 for the forward (PH_PREC_FP16X1
 * is a backward arithmetic), 0..4 for dgrad / dgrad_res / wgrad.  dgrad_res at 1x1 / stride 2 (output pixels no tap reaches)
 * takes its residual in place only (res_g == dx, res_a == NULL).  Anything else returns PH_EINVAL with nothing written.
 * ---------------------------------------------------------------------------------------------- */
size_t ph_conv2d_workspace_bytes(int B, int Cin, int IH, int IW, int Cout, int KS, int stride, int pad);
/* PH_PREC_FP16X3: the tensors a convolution READS (x of fwd / wgrad, dy of dgrad / wgrad) are half-pair tensors - layout
 * [..][C / 64][2][64] fp16 (per 64-channel slice a 128-B line of hi values, then one of lo values), 256-B aligned, C % 64 == 0
 * - and everything it writes is fp32.  These two convert (n elements, n % 64 == 0; `scale`: a power of two applied before the
 * split, 1 for activations).  Replace nothing in the reference: they are the storage format of this arithmetic. */
int ph_hp_pack(const float* src, void* dst, size_t n, float scale, ph_stream_t stream);
int ph_hp_unpack(const void* src, float* dst, size_t n, ph_stream_t stream);
int ph_conv2d_fwd(const void* x, const float* w_oihw, void* y, float* ch_sum /* [Cout] or NULL */,
                  float* ch_sumsq, int B, int Cin, int IH, int IW, int Cout, int KS, int stride, int pad, int prec,
                  void* ws, ph_stream_t stream);
int ph_conv2d_dgrad(const void* dy, const float* w_oihw, void* dx, int B, int Cin, int IH, int IW, int Cout, int KS,
                    int stride, int pad, int prec, void* ws, ph_stream_t stream);
/* dgrad with the residual term of a BasicBlock backward fused into its epilogue, as the trunk backward uses it (stride 1: the
 * identity shortcut; stride 2: the downsample path accumulates in place, res_g == dx, a parity class no tap reaches keeps dx)
 * (reference resnets.py:58-74 backward: d_x = dgrad(conv1) + d_out * (out > 0)):
 * dx = round(dgrad) + (res_a == NULL || res_a > 0 ? res_g : 0); res_g / res_a: [B][IH][IW][Cin] in the activation type. */
int ph_conv2d_dgrad_res(const void* dy, const float* w_oihw, void* dx, const void* res_g, const void* res_a, int B, int Cin,
                        int IH, int IW, int Cout, int KS, int stride, int pad, int prec, void* ws, ph_stream_t stream);
/* Test access: 3x3 stride-1 pad-1 perf-mode forward whose INPUT is the raw output of a convolution: relu(x * in_scale[c] +
 * in_shift[c]) (the BatchNorm + ReLU of reference resnets.py:58-66, rounded to bf16 as the stand-alone pass stores it) is applied to
 * every halo tile in LDS, as the forward-only networks of the distillation step run conv2 of layers 1-2. */
int ph_conv2d_fwd_fused_in(const void* x, const float* in_scale, const float* in_shift, const float* w_oihw, void* y,
                           float* ch_sum, float* ch_sumsq, int B, int Cin, int IH, int IW, int Cout, void* ws, ph_stream_t stream);
/* Test access: the same stride-1 3x3 perf-mode dgrad with the BatchNorm-backward sums of its OUTPUT taken in the epilogue
 * (the backward of `relu(bn(y))`: reference MICCAI-2022/resnets.py:58-74 through autograd - dgamma = sum dz xhat, dbeta = sum dz
 * with dz = dx * relu'), as ph_resnet_backward uses it for layer 1.  bst_y [B][IH][IW][Cin] = the BatchNorm's input y; mask =
 * (bst_a > 0) if bst_a else (bst_y * bst_scale + bst_shift > 0); sums [3][Cin] fp32 = sum dz | sum dz (bst_y - bst_mean) |
 * sum dz (bst_y2 - bst_mean2) (row 2 zero without bst_y2).  ws: ph_conv2d_workspace_bytes() + 3 * 4 * Cin * 1024 bytes. */
int ph_conv2d_dgrad_bnstat(const void* dy, const float* w_oihw, void* dx, const void* res_g, const void* res_a, const void* bst_y,
                           const void* bst_a, const void* bst_y2, const float* bst_scale, const float* bst_shift,
                           const float* bst_mean, const float* bst_mean2, float* sums, int B, int Cin, int IH, int IW, int Cout,
                           void* ws, ph_stream_t stream);
int ph_conv2d_wgrad(const void* x, const void* dy, float* dw_oihw, int B, int Cin, int IH, int IW, int Cout, int KS,
                    int stride, int pad, int prec, void* ws, ph_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * t-SVD low-rank constraint of the MIA-2022 stage-1 trainer ("MIA 2022/train_test_tSVD.py").
 * Adjacency = ph_sgemm (F F^T) + ph_l2norm_* (update_adj_tensor, :57-70).  Penalty mu/2 ||adj - aux||_F^2 (:418-431):
 *   out[0] = scale * sum (a - b)^2 ;  gradient out = gscalar[0] * alpha * (a - b).
 * ph_tsvd_update_aux replaces update_aux(adj, Lambda_global / mu) called at :382-391 (its source is absent from the
 * reference: this is the tensor-nuclear-norm proximal operator, see csrc/tsvd.hip): adj, aux are [V][B][B] (view-major),
 * V in {2,4,6,8}, B <= 512 (B <= 64: Jacobi on the embedding of X^H X; up to 128: one-sided Jacobi on the slice, one workgroup per
 * slice; up to 512: block one-sided Jacobi tiled over workgroups, one launch per round-robin step - a fixed number of launches
 * for a given (V, B), no host read, capturable); above 512 PH_EINVAL.  tnn[0] = (1/V) sum over frequency slices of the nuclear
 * norm of the thresholded slice.  ws: ph_tsvd_workspace_bytes(V, B) bytes, 16-byte aligned; its last 16 floats hold the TNN per
 * slice (0 .. V/2) and, for B > 64, the Jacobi sweeps per slice (8 ..).
 * ---------------------------------------------------------------------------------------------- */
/* Relational distillation baselines of the distiller zoo (`--distill pkt|rkd`,
 * "MIA 2022/train_test_path_multi_distill_v2.py":339-342).  Each entry returns the loss AND its gradient with respect
 * to the student rows f_s [B, D] (the teacher rows f_t are constants), fixed summation order.
 * ph_pkt_loss_grad: "MIA 2022/distiller_zoo/PKT.py":17-46 (cosine-similarity probabilities, KL, eps 1e-7).
 * ph_rkd_loss_grad: "MIA 2022/distiller_zoo/RKD.py":15-58 (w_d * smooth-L1 of mean-normalised pairwise distances +
 * w_a * smooth-L1 of the B^3 angles); one workgroup per anchor with its unit vectors and angles in LDS: 2 <= B <= 128,
 * 1 <= D <= 512 AND (B (D + 1) + B (B + 1) + B) * 4 <= 150 KiB (every B <= 128 at D = 128, B <= 105 at D = 256, B <= 81 at
 * D = 384, B <= 66 at D = 512), else PH_EINVAL before any HIP call.  ph_rkd_one_workgroup_fits is that rule for (B, D) (host only,
 * 1 / 0); a shape it refuses belongs to ph_rkd_loss_grad_part over the full anchor range.
 * ph_rkd_loss_grad_part (csrc/zoo_rkd.hip): the same loss, RKD.py:15-58, on Bg gathered rows (2 <= Bg <= 1024,
 * 1 <= D <= 512), restricted to the anchors [anchor_lo, anchor_lo + n_anchors) of the angle term (RKD.py:33-43) and to the
 * same rows of the distance matrix (RKD.py:21-31).  loss_part [1] and dx_part [Bg][D] (the gradient with respect to EVERY
 * student row) of the parts of any partition of [0, Bg) into contiguous ranges add up to the loss and gradient of the whole
 * batch; anchor_lo = 0, n_anchors = Bg is the complete loss.  The mean distances and the normalisers Bg^2 / Bg^3 are those
 * of all Bg rows; unit vectors take their norm from the row difference itself (F.normalize, eps 1e-12), so coinciding rows
 * give exact zeros and no NaN.  Fixed summation order, no atomics.  Anything outside the ranges above, anchor_lo < 0,
 * n_anchors < 1, anchor_lo + n_anchors > Bg or a NULL pointer returns PH_EINVAL before any HIP call. */
/* Cox negative partial log-likelihood of the survival task (MICCAI-2022/utils.py:361-376): loss and d loss / d theta;
 * dtheta may be NULL.  B <= 4096. */
int ph_cox_loss_grad(const float* theta, const float* survtime, const float* censor, float* loss, float* dtheta, int B,
                     ph_stream_t stream);
/* The survival task of the stage-1 teacher (MICCAI-2022/train_test_MT.py:149-152,180-203,340-458 with --task surv;
 * csrc/surv.hip).
 * ph_sigmoid_range_fwd: pred = sigmoid(hazard) * range[0] + shift[0] (networks_new.py:236-237,327-328, resnets.py:252-253),
 * sigma = sigmoid(hazard) kept for the backward; range / shift point at the module's output_range / output_shift
 * parameters in device memory.  ph_sigmoid_range_bwd: dhazard = dpred * range[0] * sigma * (1 - sigma).
 * ph_ema_update_dev: ema = hyper[3] * ema + hyper[4] * p (the EMA rate record of ph_adam_ema_step_dev) for the parameters
 * the optimiser leaves alone (output_range / output_shift: update_ema_variables, train_test_MT.py:34-38, covers them).
 * ph_surv_stage1_loss_grad: one workgroup, B <= 4096 (else PH_EINVAL).  terms[9] = cox_fuse, cox_path, cox_omic (the Cox
 * loss of utils.py:361-376 on pred, pred_path, pred_omic; one shared risk-set pass, S_i = sum_j [t_j >= t_i] exp(theta_j)),
 * kd_fuse, kd_path, kd_omic (MSE consistency against the EMA predictions, CL_utils/KD_losses.py:20-22, combined for
 * num_teachers 1 / 2 / 3 as train_test_MT.py:180-201; 0 = pred_distill off, the ema pointers may then be NULL),
 * loss_cox = cox sum, loss_pred_KD = kd_weight * kd sum, and total = lambda_cox * loss_cox + loss_pred_KD.
 * dgrad [3][B] = d total / d (pred, pred_path, pred_omic), or
 * NULL for the forward-only evaluation loss.
 * Data parallelism (the reference's nn.DataParallel computes these losses on the outputs gathered over every replica,
 * train_test_MT.py:63-64, so every risk set spans the global batch B = world * n):
 * ph_surv_pack_rows writes this replica's n rows into ONE staging block rows [8][n], quantity-major in this order:
 *   0 pred, 1 pred_path, 2 pred_omic, 3 ema_pred, 4 ema_pred_path, 5 ema_pred_omic, 6 survtime, 7 censor
 * (num_teachers 0: rows 3..5 are written as zeros and the ema pointers may be NULL).  1 <= n <= 4096.  One all-gather of
 * the block then lands the replicas' blocks rank by rank: gathered [world][8][n], global row i = row i % n of block i / n.
 * ph_surv_stage1_loss_grad_gathered reads that gathered buffer as it lands and computes the nine `terms` over the global
 * batch, and dgrad_local [3][n] = the rows rank*n .. rank*n + n - 1 of d total / d (pred, pred_path, pred_omic) (NULL:
 * forward only).  terms and dgrad_local are BITWISE what ph_surv_stage1_loss_grad computes on the concatenated vectors
 * (one shared device body, same summation order).  world >= 1, 0 <= rank < world, n >= 1, world * n <= 4096,
 * num_teachers 0..3; anything else returns PH_EINVAL before any HIP call.
 * ph_cindex_counts: lifelines' concordance_index(t, -h, e) rule (utils.py:424-425) for nvec in 1..3 risk vectors h0..h2
 * against one (survtime, event) pair: counts[v*3 + {0,1,2}] = comparable, concordant, tied pairs (exact 64-bit integers,
 * independent of row order).  Pair (i, j) is comparable iff e_i = 1 and (t_i < t_j, or t_i == t_j and e_j = 0);
 * concordant iff h_i > h_j, tied iff h_i == h_j.  2 <= N <= 1048576 (else PH_EINVAL). */
int ph_sigmoid_range_fwd(const float* hazard, const float* range, const float* shift, float* pred, float* sigma, int n,
                         ph_stream_t stream);
int ph_sigmoid_range_bwd(const float* dpred, const float* sigma, const float* range, float* dhazard, int n,
                         ph_stream_t stream);
int ph_ema_update_dev(float* ema, const float* p, size_t n, const float* hyper, ph_stream_t stream);
int ph_surv_stage1_loss_grad(const float* pred, const float* pred_path, const float* pred_omic, const float* ema_pred,
                             const float* ema_pred_path, const float* ema_pred_omic, const float* survtime,
                             const float* censor, int B, int num_teachers, float lambda_cox, float kd_weight, float* terms,
                             float* dgrad, ph_stream_t stream);
int ph_surv_pack_rows(const float* pred, const float* pred_path, const float* pred_omic, const float* ema_pred,
                      const float* ema_pred_path, const float* ema_pred_omic, const float* survtime, const float* censor, int n,
                      int num_teachers, float* rows, ph_stream_t stream);
int ph_surv_stage1_loss_grad_gathered(const float* rows, int world, int n, int rank, int num_teachers, float lambda_cox,
                                      float kd_weight, float* terms, float* dgrad_local, ph_stream_t stream);
int ph_cindex_counts(const float* survtime, const float* event, const float* h0, const float* h1, const float* h2, int nvec,
                     int N, int64_t* counts, ph_stream_t stream);
size_t ph_pkt_workspace_bytes(int B, int D);
int ph_pkt_loss_grad(const float* f_s, const float* f_t, float* loss, float* dx, int B, int D, void* workspace,
                     ph_stream_t stream);
size_t ph_rkd_workspace_bytes(int B, int D);
int ph_rkd_one_workgroup_fits(int B, int D);
int ph_rkd_loss_grad(const float* f_s, const float* f_t, float* loss, float* dx, int B, int D, float w_d, float w_a,
                     void* workspace, ph_stream_t stream);
size_t ph_rkd_part_workspace_bytes(int Bg, int D, int n_anchors);
int ph_rkd_loss_grad_part(const float* f_s, const float* f_t, int Bg, int D, int anchor_lo, int n_anchors, float w_d,
                          float w_a, float* loss_part, float* dx_part, void* workspace, ph_stream_t stream);

/* Superpixel attention masks of the MIA-2023 stage-1 trainer (SURVEY row f-4;
 * "MIA 2023/stage1_multi_modal_teacher/train_test_MT_SP_Masking.py":77-98), the part after the input gradients exist:
 * ph_superpixel_mask: grad_nchw [B,C,H,W] f32, sp_mask [B,H,W] labels in [0,N) -> mean gradient per superpixel
 * (sum over channels and pixels / (area + 1e-9); mean_out [B,N] may be NULL) and mask [B,H,W] = union of the K
 * superpixels with the largest mean (:88-93).  N <= 2048.  The reference does the aggregation on the HOST (:84-86).
 * ph_topk_threshold_mask: mask[b][i] = x[b][i] >= (K-th largest of row b)  (:96). */
int ph_superpixel_mask(const float* grad_nchw, const int64_t* sp_mask, float* mask, float* mean_out, int B, int C, int H,
                       int W, int N, int K, ph_stream_t stream);
int ph_topk_threshold_mask(const float* x, float* mask, int B, int D, int K, ph_stream_t stream);
/* out[b][c][p] = x[b][c][p] * (1 - mask[b][p])  (:201-202, the masked views; C = 1 for the omic vector) */
int ph_apply_mask(const float* x, const float* mask, float* out, int B, int C, size_t P, ph_stream_t stream);

/* Batch indices of DataLoader(shuffle=True, drop_last=True) (the training loader's sampler): rows q..q+B-1 of the keyed
 * permutation of epoch (*batch_no) / (n / B), q = ((*batch_no) % (n / B)) * B.  Distributional parity (host RNG stream). */
int ph_shuffle_indices(int64_t* out, int n, int B, uint64_t seed, const uint64_t* batch_no /* device pointer or NULL */,
                       ph_stream_t stream);

/* On-device input pipeline (reference MICCAI-2022/data_loaders_MT.py:168-175 TransformTwice(Compose([
 * RandomHorizontalFlip, RandomVerticalFlip, RandomCrop(S), ColorJitter(b, c, s, h), ToTensor, Normalize(0.5, 0.5)]))).
 * src: uint8 [n][SH][SW][3] tiles resident in HBM (the batch is rows[0..B) of it, or the first B tiles).  params: [B][2 views][16] f32 rows {flipH, flipV, top, left, brightness, contrast,
 * saturation, hue, order[4] (0 b, 1 c, 2 s, 3 h), grey mean (filled by ph_augment_apply), pad, 64-bit grey-sum accumulator (zero on entry)} - drawn on the device by
 * ph_augment_params - a counter RNG keyed by seed, *step, image and view - or supplied by the caller.  ph_augment_apply writes the
 * two views as f32 [B][3][S][S] in [-1, 1].  The colour arithmetic restates PIL / torchvision (absent here): parity
 * unpinned, see csrc/augment.hip and oracle/augment.py. */
int ph_augment_params(float* params, int B, uint64_t seed, const uint64_t* step /* device pointer or NULL */, int SH, int SW,
                      int S, float brightness, float contrast, float saturation, float hue, ph_stream_t stream);
int ph_augment_apply(const uint8_t* src, const int64_t* rows /* NULL - image b of the batch is src[b] - or src[rows[b]] */,
                     float* params, float* out0, float* out1, int B, int SH, int SW, int S, ph_stream_t stream);
/* The same pipeline with V <= 4 views per image and label maps (the loader of the MIA-2023 masking trainer,
 * "MIA 2023/stage1_multi_modal_teacher/data_loaders_MT_SP.py":352-388, :446-453: four independent views of a tile, the
 * superpixel label map carried through the flip and crop of its view).  params: [B][V][16], the row layout above.
 * ph_augment_params_v draws views 0 and 1 exactly as ph_augment_params does for the same seed and *step; views 2 and 3
 * extend the same keyed counter RNG under a key no (image, view < 2) pair of that step has.  ph_augment_apply_v: outs =
 * HOST array of V device pointers, each f32 [B][3][S][S]; label_outs = NULL or a HOST array of V device pointers (entries
 * may be NULL), each int64 [B][S][S] := sp[tile][sy][sx] under that view's flip and crop (nearest, no colour step);
 * sp: int16 [n][SH][SW] label maps next to the tiles (required where a label output is asked for).  PH_EINVAL for V
 * outside 1..4 or a crop larger than the tile, before any launch. */
int ph_augment_params_v(float* params, int B, int V, uint64_t seed, const uint64_t* step /* device pointer or NULL */, int SH,
                        int SW, int S, float brightness, float contrast, float saturation, float hue, ph_stream_t stream);
int ph_augment_apply_v(const uint8_t* src, const int16_t* sp, const int64_t* rows, float* params, float* const* outs,
                       int64_t* const* label_outs, int B, int V, int SH, int SW, int S, ph_stream_t stream);

/* SLIC superpixel segmentation on the device (the role of fast_slic in the reference,
 * data_loaders_MT_SP.py:303-304 - same interface, NOT bit parity: its source is not available).  All-integer definition
 * (table-driven 8-bit CIELAB, 64-bit distances, lowest label on a tie, integer sums): exactly reproducible, equal to
 * tests/slic_emulation.py on every pixel.  Grid gy = floor(sqrt(K H / W)), gx = K / gy, N = gy gx <= K labels.
 * ph_slic_num_labels: N, or PH_EINVAL for K < 1, an empty image, H or W > 8192, a grid finer than the pixels or
 * N > 2048 (the limit of ph_superpixel_mask).  Host only.
 * ph_slic_workspace_bytes: bytes of workspace ph_slic needs for n tiles (0 for invalid arguments).  Host only.
 * ph_slic_lab: rgb uint8 [npix][3] -> packed 8-bit Lab words L | a << 8 | b << 16 (L * 255 / 100, a + 128, b + 128);
 * workspace: at least the bytes ph_slic_workspace_bytes gives for one 1 x 1 tile (the two conversion tables are
 * uploaded into it).
 * ph_slic: tiles uint8 [n][H][W][3] -> labels int16 [n][H][W] in [0, N) after `iters` iterations at the given
 * compactness (0..1024); one fixed launch sequence on `stream`, no host synchronisation. */
int ph_slic_num_labels(int H, int W, int K);
size_t ph_slic_workspace_bytes(int n, int H, int W, int K);
int ph_slic_lab(const uint8_t* rgb, uint32_t* lab, size_t npix, void* workspace, ph_stream_t stream);
int ph_slic(const uint8_t* tiles, int16_t* labels, int n, int H, int W, int K, int compactness, int iters, void* workspace,
            ph_stream_t stream);
/* Connectivity pass over int16 label maps [n][H][W] with labels in [0, N) (a rule of this project's
 * own, integers only, independent of the order of evaluation, equal to tests/slic_connect_emulation.py on every pixel).
 * A component is a maximal 4-connected set of pixels of one label; its first pixel is its lowest raster index y W + x.
 * The principal component of a label is its largest (tie: the lowest first pixel) and is never relabelled.  A component
 * that is not principal, has fewer than min_size pixels and does not start at pixel (0, 0) takes the final label of the
 * component that holds the pixel above its first pixel (in row 0: the pixel to its left); every other component keeps
 * its label.  The rule is applied once; min_size = 1 is the identity.  A pixel whose label lies outside [0, N) indexes
 * no table: its component keeps its label.
 * Bounds: 1 <= n <= 65535, 1 <= H, W <= 8192, 1 <= N <= 2048, min_size >= 1, non-NULL pointers; anything else is
 * PH_EINVAL (the workspace size: 0) before any launch.  labels_in == labels_out is allowed.  Seven kernels on `stream`,
 * a fixed sequence without a host read (capturable).  Workspace: two 32-bit words per pixel and one 64-bit word per
 * label and tile, as ph_slic_connect_workspace_bytes says (host only). */
size_t ph_slic_connect_workspace_bytes(int n, int H, int W, int N);
int ph_slic_connect(const int16_t* labels_in, int16_t* labels_out, int n, int H, int W, int N, int min_size, void* workspace,
                    ph_stream_t stream);

/* On-device contrast-index sampler (reference MICCAI-2022/data_loaders_MT.py:229-249 and the neg_mode
 * variants of "MIA 2023/stage2_unimodal_student/data_loaders_MT.py":205-238).  out[b] = [positives | K negatives]:
 * pos_mode 0 'exact' (the query), 1 'relax' (one same-class row), 2 'multi_pos' (P distinct same-class rows, slot 0 :=
 * the query); neg_mode 0 'diff_class' (rows of the other classes), 1 'all_others' (every row but the query); with
 * replacement exactly when K exceeds the candidate list.  cls_pos / cls_neg: the per-class row lists concatenated,
 * *_off[c] .. *_off[c+1] delimiting class c.  `step` (device counter, may be NULL) and `seed` select the draw. */
int ph_contrast_sampler(const int64_t* index, const int64_t* grade, const int* cls_pos, const int* cls_pos_off,
                        const int* cls_neg, const int* cls_neg_off, int n_data, int B, int P, int K, int pos_mode,
                        int neg_mode, uint64_t seed, const uint64_t* step, int64_t* out, ph_stream_t stream);

/* ContrastMemory_v3.forward called WITHOUT contrast indices (reference MICCAI-2022/CL_utils/memory_new.py:265-267:
 * `idx = self.multinomial.draw(batchSize * (self.K + P)).view(batchSize, -1); idx.select(1, 0).copy_(y.data)`, AliasMethod
 * :401-458 over uniform unigrams): out [B][S] int64, column 0 = y[b], every other entry uniform in [0, n_data) with
 * replacement.  `seed` and the device counter `step` (may be NULL) select the draw; distributional parity. */
int ph_alias_uniform_draw(const int64_t* y, int64_t* out, int n_data, int B, int S, uint64_t seed, const uint64_t* step,
                          ph_stream_t stream);

/* Orthogonality loss of the stage-1 trainer (reference MICCAI-2022/CL_utils/orthogonal_loss.py:18-32): rows scaled by
 * a DETACHED 1/(||x||+eps) (:24-28); the D x D cross-correlation and its mean square are ph_sgemm + ph_sqdiff_sum. */
int ph_row_invnorm_scale(const float* x, float* y, float* inv /* [B] */, int B, int D, float eps, ph_stream_t stream);
int ph_row_scale(const float* x, const float* r /* [B] */, float* y, int B, int D, ph_stream_t stream);
int ph_sqdiff_sum(const float* a, const float* b, float* out, size_t n, float scale, ph_stream_t stream);
int ph_scaled_diff(const float* a, const float* b, const float* gscalar, float alpha, float* out, size_t n,
                   ph_stream_t stream);
/* the mixed-feature views of n_views = 6 / 8 (:305-307, :334-363): out = wa * a / max(a) + wb * b / max(b) over n elements */
int ph_maxnorm_mix(const float* a, const float* b, float* out, size_t n, float wa, float wb, ph_stream_t stream);
size_t ph_tsvd_workspace_bytes(int V, int B);
int ph_tsvd_update_aux(const float* adj, float* aux, float* tnn /* may be NULL */, int V, int B, float tau,
                       void* workspace, ph_stream_t stream);
/* the same with tau = tau_dev[0] read on the device (a HIP graph of the stage-1 step replays with the current mu) */
int ph_tsvd_update_aux_dev(const float* adj, float* aux, float* tnn /* may be NULL */, int V, int B, const float* tau_dev,
                           void* workspace, ph_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The tail of the patch-level test pass: nine overlapping patches per test ROI
 * (data_loaders_MT.py:67-77, train_test_path_multi_distill.py:360-366, "MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":489-492), scored per
 * patch and per patient.  The reference copies every prediction row to the host and calls sklearn / pandas there.
 *
 * ph_rank_counts: micro-averaged roc_auc_score and average_precision_score (core/utils_analysis.py:160-161,
 * train_test_path_multi_distill.py:516-526) as exact counts.  pred f32 [N][C], grade int64 [N]; the M = N * C pairs
 * (score pred[n][c], label grade[n] == c) are compared all against all (j side staged in LDS in tiles of 256).
 * counts int64 [4] = {P, concordant, tied, bad}: P positives; concordant / tied = the (positive i, negative j) pairs with
 * s_i > s_j / s_i == s_j; bad = non-finite scores + labels outside [0, C).  ap_sum float64 [1] = the sum over the positives
 * of ge_pos_i / ge_all_i (ge_all_i = #{j: s_j >= s_i}, ge_pos_i the positives among them), added in a fixed order (a tree
 * over each block of 256 pairs, then block t, t + 256, .. per thread and the same tree): two runs agree bitwise.
 * With Q = M - P:  AUC = (concordant + tied / 2) / (P Q),  AP = ap_sum / P - sklearn's values, ties included.  Integer totals
 * by 64-bit atomics: exact, independent of the order.  N >= 1, C >= 1, M <= 1048576; workspace: the bytes
 * ph_rank_counts_workspace_bytes gives (0 for a refused shape; host only).
 * ph_confusion_counts: conf int64 [C][C], row = grade[n], column = arg-max of pred[n] (the FIRST maximum, as np.argmax) -
 * the integers behind f1_score(average="micro" | None) (utils_analysis.py:162-163) and the accuracy.  A row whose label lies
 * outside [0, C) is left out.  N >= 1, 1 <= C <= 16.
 * ph_group_agg: the per-patient groupby('TCGA ID').agg(fun) of utils_analysis.py:123.  x f32 [N][C]; the groups as a CSR
 * built by the caller: offsets int32 [G + 1], order int32 [N] (the rows of group g are order[offsets[g]] ..
 * order[offsets[g + 1] - 1], ascending; groups need not be contiguous in x); out f32 [G][C].  PH_AGG_MEAN: float64 sum in
 * that order, divided by the count, rounded to float32 once.  PH_AGG_MAX: exact, starting from -inf.  offsets_host is the
 * HOST copy of offsets: it is checked before the launch (offsets[0] = 0, offsets[G] = N, no empty group - else PH_EINVAL).
 * 1 <= G <= N <= 16777216, 1 <= C <= 4096.
 * All three return PH_EINVAL for a NULL pointer or a size outside the stated range before any HIP call.
 *
 * ph_group_quantile: the order statistics of the same groups - the median of the survival
 * aggregation (utils_analysis.py:467) and the percentile form of the grading one (:122) - over the CSR of ph_group_agg.
 * For one (group, column) with n values, s = the values ascending:  h = (n - 1) q in double, lo = floor(h),
 * hi = min(lo + 1, n - 1), t = h - lo, a = s[lo], b = s[hi];  out = (float)(t == 0 || a == b ? a : a + (b - a) t), evaluated
 * in double (a product and a sum, not fused) and rounded once: numpy's percentile with method "linear"; q = 0.5 is pandas'
 * median, q = 0 the minimum, q = 1 the maximum.  A NaN anywhere in the group's column gives NaN; +-inf are ordinary values
 * and the expression gives what IEEE gives; the sign of a zero among mixed +-0 is unspecified.  No sort: the element whose
 * stable rank (#{smaller} + #{equal and earlier in CSR order}) is lo hands over a, the one of rank hi hands over b - one
 * launch, no workspace, no atomics, independent of scheduling.  The form is chosen per launch from the largest group of
 * offsets_host: at most 64 rows - one 64-lane wave per (group, column); more - one workgroup of 256 per group, the column
 * staged in LDS.  The kernels clamp the device offsets and skip a row index outside [0, N).
 * The limits of ph_group_agg, and every group at most PH_QUANTILE_MAX_GROUP rows, and 0 <= q <= 1 (a NaN q is refused);
 * anything else, a NULL pointer or an empty group returns PH_EINVAL before any HIP call.
 *
 * ph_rank_counts_classes: the one-vs-rest counts of EVERY column in one call - what
 * roc_auc_score / average_precision_score(average="macro" | "weighted" | None) are made of (calcGradMetrics /
 * calcAggGradMetrics(..., avg), core/utils_analysis.py:138-167).  Class c: element n has score pred[n][c] and label
 * grade[n] == c.  counts int64 [C][4] = {P_c, concordant_c, tied_c, bad_c} as ph_rank_counts defines them over the N elements
 * of the column; bad_c = the non-finite scores of column c, and for c == 0 also the labels outside [0, C).  ap_sum float64
 * [C]: the sum of ge_pos / ge_all over the positives of column c, added in the fixed order of ph_rank_counts (a tree over each
 * block of 256 ROWS, then block t, t + 256, .. per thread and the same tree): two runs agree bitwise.  With Q_c = N - P_c:
 * AUC_c = (concordant_c + tied_c / 2) / (P_c Q_c), AP_c = ap_sum_c / P_c.  A row is a positive of its own class only, so
 * thread = row n compares pred[n][grade[n]] with that column of every row; one workgroup stages its 256 x C tile once for
 * all classes.  1 <= N <= 1048576, 1 <= C <= 16; workspace: ph_rank_counts_classes_workspace_bytes (0 for a refused shape).
 * A memset and two launches whatever C is; no host read.
 *
 * ph_roc_points (section 26): the integer points of roc_curve (makeAUROCPlot, core/utils_analysis.py:172-215) at every
 * distinct threshold.  cls in [0, C): the one-vs-rest problem of that column, M = N elements, element n with score
 * pred[n][cls] and label grade[n] == cls.  cls == -1: the micro problem over the M = N * C pairs in the pair order of ph_rank_counts.  For the
 * k-th largest distinct score t_k:  thr[k] = t_k,  tps[k] = #{positive j: s_j >= t_k},  fps[k] = #{negative j: s_j >= t_k}
 * (int32), k = 0 .. npoints[0] - 1; entries from npoints[0] on are left unwritten.  npoints int32 [2]: [0] the number of
 * points, [1] the bad count (non-finite scores and labels outside [0, C), a label once per row).  A NaN score compares false
 * everywhere and takes part in nothing; +-inf are ordinary scores.  No sort: element i represents its score when no EARLIER
 * element has an equal one, and its slot is the number of representatives with a larger score - two all-pairs passes over LDS
 * tiles of 256, integers and copied floats only: bit for bit independent of scheduling.  fps, tps, thr hold M entries each.
 * 1 <= N <= 1048576, 1 <= C <= 16, M <= 1048576; workspace: ph_roc_points_workspace_bytes = 12 bytes per element of the
 * largest problem the shape admits (N * C, or N where N * C > 1048576 and only cls >= 0 is served; 0 for a refused shape).
 * A memset and two launches; no host read.
 * Both return PH_EINVAL for a NULL pointer, a size outside the stated range or a cls outside [-1, C) before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
#define PH_AGG_MEAN 0
#define PH_AGG_MAX 1
#define PH_QUANTILE_MAX_GROUP 4096
size_t ph_rank_counts_workspace_bytes(int N, int C);
int ph_rank_counts(const float* pred, const int64_t* grade, int N, int C, int64_t* counts, double* ap_sum, void* workspace,
                   ph_stream_t stream);
int ph_confusion_counts(const float* pred, const int64_t* grade, int N, int C, int64_t* conf, ph_stream_t stream);
int ph_group_agg(const float* x, const int32_t* offsets, const int32_t* order, const int32_t* offsets_host, int N, int C, int G,
                 int fun, float* out, ph_stream_t stream);
int ph_group_quantile(const float* x, const int32_t* offsets, const int32_t* order, const int32_t* offsets_host, int N, int C,
                      int G, double q, float* out, ph_stream_t stream);
size_t ph_rank_counts_classes_workspace_bytes(int N, int C);
int ph_rank_counts_classes(const float* pred, const int64_t* grade, int N, int C, int64_t* counts, double* ap_sum,
                           void* workspace, ph_stream_t stream);
size_t ph_roc_points_workspace_bytes(int N, int C);
int ph_roc_points(const float* pred, const int64_t* grade, int N, int C, int cls, int32_t* fps, int32_t* tps, float* thr,
                  int32_t* npoints, void* workspace, ph_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The survival side of the patient-level test pass: risk strata, the event table per stratum, the
 * log-rank sums between strata and the Kaplan-Meier estimate per stratum (core/utils_analysis.py:259-263, :398-418, :719-780;
 * numpy and lifelines on the host there).  No sort: ranks and slots are exact counts from all-pairs passes over LDS tiles
 * of 256; each entry is a fixed number of memsets and launches whatever N is, and reads nothing back.
 *
 * ph_surv_strata: hazard f32 [N] (device); q double [K] (HOST, percent).  cuts double [K] (device):
 * cuts[i] = np.percentile(hazard.astype(float64), q[i]), method "linear", restated exactly:  h = (N - 1) (q / 100) in double,
 * lo = floor(h), hi = min(lo + 1, N - 1), t = h - lo, a and b the values of stable rank lo and hi (#{smaller} + #{equal and
 * earlier}, counted over the whole vector);  t == 0 or a == b: a;  t < 0.5: a + (b - a) t;  else b - (b - a) (1 - t) - numpy's
 * _lerp with both of its forms, products and sums unfused, never rounded to float32.  (One divergence: with t == 0 or a == b
 * numpy still evaluates a + (b - a) t and returns NaN when a or b is infinite; this entry returns a.  Finite order statistics
 * give numpy's bits.)  Then the reference's patch (:412, :722):
 * K == 2 and cuts[0] == cuts[1] sets cuts[0] = 2.99997.  group int32 [N]: the FIRST i with (double)hazard[n] < cuts[i], else K
 * (the first-i rule of hazard2grade, not a count of cuts: the patch can leave the cuts non-ascending).  sizes int32 [K + 1]: the rows per group.
 * bad int32 [1]: the non-finite hazards.  A NaN hazard makes every cut NaN (numpy's rule) and every row falls in group K;
 * +-inf are ordinary values and the expression gives what IEEE gives.  2 <= N <= 1048576, 1 <= K <= 7, every q finite in
 * [0, 100]; workspace: ph_surv_strata_workspace_bytes = 64.  Three memsets and two launches.
 *
 * ph_surv_table: lifelines' event table per group over every distinct observed time (event or censored), ascending.
 * survtime, event f32 [N] (an event is event > 0), group int32 [N], G groups.  For slot k with time times[k]:
 * at_risk[k][g] = #{j in g: t_j >= times[k]}, observed[k][g] = #{j in g: t_j == times[k], event}, censored[k][g] the same for
 * the rows with no event (int32 [N][G] each, times f32 [N]); k = 0 .. npoints[0] - 1, entries from npoints[0] on are left
 * unwritten.  npoints int32 [2]: [0] the number of slots, [1] the rows that take part in nothing (group outside [0, G) or a
 * NaN time).  A row represents its time when no EARLIER row has an equal one; its slot is the number of representatives with
 * a smaller time.  Integers and copied floats only: bit for bit independent of scheduling and of the row order.  Times compare
 * as float32.  2 <= N <= 1048576, 1 <= G <= 8; workspace: ph_surv_table_workspace_bytes = 4 N.  A memset and two launches.
 *
 * ph_surv_logrank_km: from the table (at_risk, observed, npoints on the device; N = the capacity of the arrays).
 * pairs int32 [P][2] (HOST): for pair (a, b) the log-rank test over the members of a and b only - per slot, with
 * n = n_a + n_b and d = d_a + d_b, where d > 0:  O - E += d_a - (d n_a) / n,  and for n > 1
 * V += n_a (n - n_a) d (n - d) / (n n (n - 1))  (float64, evaluated left to right as written);  stat double [P][2] = (O - E, V),
 * chi2 = (O - E)^2 / V with one degree of freedom.  The sums have a fixed shape (a tree over each tile of 256 slots, then tile
 * t, t + 256, .. per thread and the same tree): two runs agree bitwise.  surv double [N][G]:
 * surv[k][g] = prod over j <= k with at_risk[j][g] > 0 of (1 - observed[j][g] / at_risk[j][g]), the Kaplan-Meier estimate at
 * every slot (the product of the tiles before, then the slots of the tile in order); entries from npoints[0] on are left
 * unwritten.  Limits of ph_surv_table, 0 <= P <= 28 (pairs and stat may be NULL when P == 0), every pair index in [0, G) and
 * a != b; workspace: ph_surv_logrank_km_workspace_bytes = 8 ceil(N / 256) (2 P + 2 G).  Three launches.
 *
 * All three return PH_EINVAL for a NULL pointer or a value outside the stated ranges before any HIP call, and each
 * workspace query returns 0 for a refused shape.
 * ---------------------------------------------------------------------------------------------- */
size_t ph_surv_strata_workspace_bytes(int N, int K);
int ph_surv_strata(const float* hazard, int N, const double* q, int K, double* cuts, int32_t* group, int32_t* sizes, int32_t* bad,
                   void* workspace, ph_stream_t stream);
size_t ph_surv_table_workspace_bytes(int N, int G);
int ph_surv_table(const float* survtime, const float* event, const int32_t* group, int N, int G, float* times, int32_t* at_risk,
                  int32_t* observed, int32_t* censored, int32_t* npoints, void* workspace, ph_stream_t stream);
size_t ph_surv_logrank_km_workspace_bytes(int N, int G, int P);
int ph_surv_logrank_km(const int32_t* at_risk, const int32_t* observed, const int32_t* npoints, int N, int G, const int32_t* pairs,
                       int P, double* stat, double* surv, void* workspace, ph_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Between the batch body and the test pass of the stage-2 trainers' train(): the epoch bookkeeping,
 * the MIA-2023 per-sample stores and the similarity audit over them - all on the device, no float atomics, every float64 sum
 * in a fixed order (two runs agree bitwise).
 *
 * ph_epoch_record_add: ONE launch (capturable in a HIP graph) that adds a step into a persistent record of
 * PH_EPOCHREC_WORDS 8-byte words, which the caller zeroes with a memset at epoch start and reads once at epoch end:
 *   words [0, 16)   float64: sum k of the device scalars.  scalars (HOST array of n_scalars DEVICE pointers to one float32
 *                   each) and modes (HOST int32 [n_scalars]) are read at the call; scalar k is read on the device when the
 *                   stream gets there, widened to float64 and added - in call order, so the sum equals Python's
 *                   `acc += t.item()` bit for bit.  PH_REC_ADD: always (a NaN propagates).  PH_REC_ADD_POSITIVE: only when the
 *                   value is > 0.0 (`if loss_div > 0.0:`, MICCAI-2022 train_test_path_multi_distill.py:320-324) - 0.0, -0.0, a
 *                   negative value and a NaN are not added.
 *   words [16, 32)  float64: the elementwise sum of wvec f32 [n_w] (`loss_weights += scale`, :305).
 *   words [32, 34)  float64: the sum over the calls of mean(row0) and mean(row1), f32 [n_row] each (row1 may be NULL, both
 *                   may be): the row added in float64 (element t, t + 256, .. per thread, then a fixed tree), divided by
 *                   n_row ("MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":380-383, :475-476).
 *   word 34         int64: rows of pred f32 [B][C] whose arg-max (the FIRST maximum, as ph_confusion_counts) equals grade[b];
 *   word 35         int64: rows whose label lies outside [0, C) - left out of word 34;   word 37: int64, the rows seen (+= B).
 *   word 36         int64: the calls (steps).
 *   words [40, 56)  int64: how often scalar k was added (under PH_REC_ADD_POSITIVE: the calls whose value passed the test).
 * pred and grade are both NULL or both given.  0 <= n_scalars, n_w <= 16; with pred 1 <= B <= 1048576, 1 <= C <= 16; with
 * row0 1 <= n_row <= 1048576.  A call with nothing to add is refused.
 *
 * ph_store_rows: store[index[b]] = rows[b] for the B rows of rows f32 [B][D] (softmax == 1: softmax over the row first,
 * float32, max-subtracted), store f32 [n][D], index int64 [B].  An index outside [0, n) is skipped and counted in
 * skipped int64 [1] (+=; the caller zeroes it).  Among equal indices of one batch the HIGHEST position b wins, as numpy's
 * a[index] = rows.  1 <= B <= 65536, 1 <= D <= 4096, 1 <= n <= 2^31.  One launch, capturable.
 *
 * ph_sim_audit: evaluate_feature / evaluate_logits (:162-196) over F f32 [n][Df] (teacher) and P f32 [n][Dp] (student),
 * labels int64 [n] (NULL: one class).  With S_f, S_p the cosine similarity matrices (rows scaled by 1 / |row|, the norm from a
 * float64 sum of squares; a zero row has similarity 0 with everything, as sklearn's normalize):
 *   sums double [5]   = sum of S_f over the intra-class ordered pairs, over the inter-class ones, the same two of S_p,
 *                       and sum |S_f - S_p| over all n^2 pairs (the difference in float32, as numpy's);
 *   counts int64 [2]  = intra-class pairs, inter-class pairs.  Pairs are ordered and include the diagonal (np.equal).
 * The host divides (no inter-class pair: 0 / 0 = NaN, numpy's mean of an empty selection).  No n x n matrix: workgroup
 * (tile of 64 rows i, range of j tiles) streams tiles of 64 rows j, both Gram tiles by exact-f32 MFMA 32x32x2 over zero-padded
 * chunks of 32 columns, class test and sums in the epilogue, per-workgroup float64 partials added in a fixed order.
 * 1 <= n <= 65536, 1 <= Df, Dp <= 512; workspace (256-byte aligned): ph_sim_audit_workspace_bytes (0 for a refused shape).
 * One memset and three launches whatever n is; no host read.
 *
 * ph_stage1_record_add: the same for the stage-1 teacher step.  ONE launch of ONE workgroup
 * (capturable) that adds a step into a persistent record of PH_STAGE1REC_WORDS 8-byte words, zeroed by the caller with a
 * memset at epoch start and read once at epoch end:
 *   words [0, 16)   float64: sum k of the device scalars - scalars / modes / n_scalars exactly as ph_epoch_record_add takes
 *                   them, by the same device routine: widened to float64, added in call order, PH_REC_ADD / PH_REC_ADD_POSITIVE.
 *   words [16, 32)  int64: how often scalar k was added.
 *   words [32, 35)  int64: per head h < n_heads the rows of pred_h f32 [B][C] whose arg-max (the FIRST maximum, as word 34 of
 *                   the stage-2 record and ph_confusion_counts) equals grade[b], int64 [B].  Exactly the first n_heads of
 *                   pred0..pred2 are given, the others NULL; grade is given iff n_heads > 0.
 *   word 35         int64: rows whose label lies outside [0, C) - counted ONCE per row and left out of every head's count.
 *   word 36         int64: the calls (steps);   word 37: int64, the rows seen (+= B when heads or survival rows are given).
 *   word 38         int64: the CURSOR of the survival store = the rows appended since the memset.
 *   word 39         int64: overflow = the rows dropped because the store was full.
 *   words [40, 48)  spare (left zero).
 * Survival rows: h_fuse, h_path, h_omic, censor, survtime f32 [B] and store f32 [5][cap] - all six pointers given, or none.
 * Row b of the step goes to column cursor + b of the store (store[k * cap + cursor + b], k in the order above) while that is
 * < cap; the rows that do not fit are dropped and counted in word 39; nothing is written at or past cap, whatever word 38
 * holds.  The cursor lives in the record: the memset rewinds it, and a replayed graph appends at the right place without any
 * per-step host value.  Every thread reads the cursor before a workgroup barrier and thread 0 advances it after it - one
 * workgroup, so no ordering between blocks is relied on.
 * 0 <= n_scalars <= 16, 0 <= n_heads <= 3; with heads or survival rows 1 <= B <= 65536; with heads 1 <= C <= 16; with survival
 * rows 1 <= cap <= 1048576 (the range of ph_cindex_counts).  record 8-byte aligned, grade 8-byte, every float pointer 4-byte.
 * A call with nothing to add, or with the survival pointers given only in part, is refused.
 *
 * All return PH_EINVAL for a NULL pointer (where not stated optional), a misaligned pointer or a size outside the stated
 * range before any HIP call; nothing is written then.
 * ---------------------------------------------------------------------------------------------- */
#define PH_STAGE1REC_WORDS 48
int ph_stage1_record_add(void* record, const float* const* scalars, const int32_t* modes, int n_scalars, const float* pred0,
                         const float* pred1, const float* pred2, int n_heads, const int64_t* grade, int B, int C,
                         const float* h_fuse, const float* h_path, const float* h_omic, const float* censor,
                         const float* survtime, float* store, int cap, ph_stream_t stream);
#define PH_EPOCHREC_WORDS 56
#define PH_EPOCHREC_MAX_SCALARS 16
#define PH_REC_ADD 0
#define PH_REC_ADD_POSITIVE 1
int ph_epoch_record_add(void* record, const float* const* scalars, const int32_t* modes, int n_scalars, const float* wvec,
                        int n_w, const float* pred, const int64_t* grade, int B, int C, const float* row0, const float* row1,
                        int n_row, ph_stream_t stream);
int ph_store_rows(const float* rows, const int64_t* index, int B, int D, float* store, int64_t n, int softmax,
                  int64_t* skipped, ph_stream_t stream);
size_t ph_sim_audit_workspace_bytes(int n, int Df, int Dp);
int ph_sim_audit(const float* F, const float* P, const int64_t* labels, int n, int Df, int Dp, double* sums, int64_t* counts,
                 void* workspace, ph_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * In-library kernel timer for bench.py's `roofline` object: HIP events around every MFMA kernel launch on the
 * launch stream.  Classes: 0 first-generation tap-conv Cout=64 (dgrad parity classes), 1 first-generation tap-conv
 * Cout>=128 stride 1 (1x1, dgrad parity classes), 2 tap-conv stride 2, 3 wgrad, 4 stem forward, 5 stem wgrad,
 * 6 tapconv2 3x3 stride-1 Cout>=128 (fwd + dgrad), 7 tapconv2 3x3 stride-1 Cin=Cout=64 (layer 1).
 * out[cls*3 + {0,1,2}] = {launches, total ms, total algorithmic work}; 12 classes: 0-7 the MFMA kernels (work = FLOPs),
 * 8-11 the HBM-bound crd_score / crd_loss_grad / adam_ema / bn_apply kernels (work = algorithmic bytes).
 * ---------------------------------------------------------------------------------------------- */
int ph_prof_enable(int on);
int ph_prof_reset(void);
int ph_prof_summary(double* out, int nclasses);
/* out[cls*4 + {0,1,2,3}] = {launches, total ms, total algorithmic work, total algorithmic HBM bytes} */
int ph_prof_summary4(double* out, int nclasses);
/* Phase marker: a one-thread launch that stores the device's 100 MHz wall clock into *out (device memory) when `stream`
 * reaches it - capturable in a HIP graph, unlike events, so the phases of a replayed step can be timed. */
int ph_prof_stamp(unsigned long long* out, ph_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PATHOMIC_HIP_H_ */
