#pragma once
#include <ATen/ATen.h>
#include <c10/util/Optional.h>

#include <string>
#include <tuple>
#include <vector>

namespace cdp {

void set_conv_gemm(const std::string& mode);
// tuning sweeps: force the tile / split-K plan of later conv ('conv') or weight-gradient ('wgrad')
// GEMMs (0 = planner's choice); plan_info returns the planner's {bm, bn, splits}
int64_t pair_launches();
void set_gemm_override(const std::string& kind, int64_t bm, int64_t bn, int64_t splits);
std::vector<int64_t> plan_info(const std::string& kind, int64_t M, int64_t N, int64_t K);
std::string get_conv_gemm();
std::vector<at::Tensor> conv2d_fwd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                                   int64_t stride, int64_t pad, bool want_stats,
                                   const c10::optional<at::Tensor>& x_amax = c10::nullopt,
                                   const c10::optional<at::Tensor>& w_amax = c10::nullopt);
at::Tensor conv2d_dgrad(const at::Tensor& dy, const at::Tensor& w, std::vector<int64_t> in_shape, int64_t stride,
                        int64_t pad, const c10::optional<at::Tensor>& addend,
                        const c10::optional<at::Tensor>& dy_amax = c10::nullopt,
                        const c10::optional<at::Tensor>& w_amax = c10::nullopt,
                        const c10::optional<at::Tensor>& w_t = c10::nullopt);
at::Tensor conv2d_wgrad(const at::Tensor& dy, const at::Tensor& x, std::vector<int64_t> w_shape, int64_t stride,
                        int64_t pad, const c10::optional<at::Tensor>& out, bool accumulate,
                        const c10::optional<at::Tensor>& dy_amax = c10::nullopt,
                        const c10::optional<at::Tensor>& x_amax = c10::nullopt);
at::Tensor conv2d_wgrad_keep(const at::Tensor& dy, const at::Tensor& x, std::vector<int64_t> w_shape, int64_t stride,
                             int64_t pad, const c10::optional<at::Tensor>& out, bool accumulate, int64_t keep_c,
                             const c10::optional<at::Tensor>& dy_amax = c10::nullopt,
                             const c10::optional<at::Tensor>& x_amax = c10::nullopt);
std::vector<at::Tensor> conv_bn_act_fwd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& b,
                                        const c10::optional<at::Tensor>& gamma, const c10::optional<at::Tensor>& beta,
                                        const c10::optional<at::Tensor>& running_mean,
                                        const c10::optional<at::Tensor>& running_var,
                                        const c10::optional<at::Tensor>& num_batches_tracked, double momentum,
                                        double eps, bool training, int64_t stride, int64_t pad, bool pool, bool relu,
                                        const c10::optional<at::Tensor>& residual,
                                        const c10::optional<at::Tensor>& x_amax = c10::nullopt,
                                        const c10::optional<at::Tensor>& w_amax = c10::nullopt,
                                        const c10::optional<at::Tensor>& res_y = c10::nullopt,
                                        const c10::optional<at::Tensor>& res_stats = c10::nullopt,
                                        bool defer_apply = false,
                                        const c10::optional<at::Tensor>& drop_scale = c10::nullopt);
at::Tensor act_max_of(const at::Tensor& t);
int64_t act_max_memsets();
int64_t act_max_copies();
std::vector<std::vector<at::Tensor>> weight_prep(const std::vector<at::Tensor>& ts, const std::vector<bool>& want_t);
void weight_prep_into(const std::vector<at::Tensor>& ts, const std::vector<bool>& want_t, const at::Tensor& amax,
                      const std::vector<c10::optional<at::Tensor>>& wts);
std::vector<at::Tensor> conv_bn_act_bwd(const at::Tensor& gout, const at::Tensor& x, const at::Tensor& w,
                                        const at::Tensor& y, const at::Tensor& stats, int64_t stride, int64_t pad,
                                        bool pool, bool relu, bool need_dx, bool has_bias,
                                        const c10::optional<at::Tensor>& zout, bool training,
                                        const c10::optional<at::Tensor>& dw_out,
                                        const c10::optional<at::Tensor>& db_out,
                                        const c10::optional<at::Tensor>& dgamma_out,
                                        const c10::optional<at::Tensor>& dbeta_out,
                                        const c10::optional<at::Tensor>& dx_addend,
                                        const c10::optional<at::Tensor>& x_amax = c10::nullopt,
                                        const c10::optional<at::Tensor>& w_amax = c10::nullopt,
                                        const c10::optional<at::Tensor>& w_t = c10::nullopt,
                                        const c10::optional<at::Tensor>& part_in = c10::nullopt,
                                        const c10::optional<at::Tensor>& prev_y = c10::nullopt,
                                        const c10::optional<at::Tensor>& prev_stats = c10::nullopt,
                                        bool prev_pool = false, bool prev_relu = false, int64_t prev_ps = 2,
                                        const c10::optional<at::Tensor>& bias = c10::nullopt,
                                        const c10::optional<at::Tensor>& drop_scale = c10::nullopt);
at::Tensor linear_fwd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& b);
std::vector<at::Tensor> linear_bwd(const at::Tensor& gy, const at::Tensor& x, const at::Tensor& w, bool need_dx,
                                   bool has_bias, const c10::optional<at::Tensor>& dw_out,
                                   const c10::optional<at::Tensor>& db_out);
// target_b + lam (both or neither): the two-target loss of mixup / CutMix, lam a 1-element fp32 device tensor
at::Tensor xent_fwd(const at::Tensor& logits, const at::Tensor& target, const c10::optional<at::Tensor>& correct,
                    double label_smoothing = 0.0, int64_t topk = 1,
                    const c10::optional<at::Tensor>& target_b = c10::nullopt,
                    const c10::optional<at::Tensor>& lam = c10::nullopt);
at::Tensor xent_bwd(const at::Tensor& gloss, const at::Tensor& logits, const at::Tensor& target,
                    double label_smoothing = 0.0, const c10::optional<at::Tensor>& target_b = c10::nullopt,
                    const c10::optional<at::Tensor>& lam = c10::nullopt);
std::vector<at::Tensor> xent_linear_bwd(const at::Tensor& gloss, const at::Tensor& logits, const at::Tensor& target,
                                        const at::Tensor& x, const at::Tensor& w, bool need_dx, bool has_bias,
                                        const c10::optional<at::Tensor>& dw_out, const c10::optional<at::Tensor>& db_out,
                                        const c10::optional<at::Tensor>& link_y = c10::nullopt,
                                        const c10::optional<at::Tensor>& link_stats = c10::nullopt,
                                        bool link_pool = false, bool link_relu = false, int64_t link_ps = 2,
                                        double label_smoothing = 0.0,
                                        const c10::optional<at::Tensor>& target_b = c10::nullopt,
                                        const c10::optional<at::Tensor>& lam = c10::nullopt, bool bce = false,
                                        const c10::optional<double>& target_threshold = c10::nullopt,
                                        bool sum_classes = false);
// Binary cross-entropy with logits over index and mixed targets (mean over B * C; sum_classes: over B);
// target_threshold in [0, 1): the dense target is y > target_threshold
at::Tensor bce_fwd(const at::Tensor& logits, const at::Tensor& target, double label_smoothing = 0.0,
                   const c10::optional<double>& target_threshold = c10::nullopt, bool sum_classes = false,
                   const c10::optional<at::Tensor>& target_b = c10::nullopt,
                   const c10::optional<at::Tensor>& lam = c10::nullopt);
at::Tensor bce_bwd(const at::Tensor& gloss, const at::Tensor& logits, const at::Tensor& target,
                   double label_smoothing = 0.0, const c10::optional<double>& target_threshold = c10::nullopt,
                   bool sum_classes = false, const c10::optional<at::Tensor>& target_b = c10::nullopt,
                   const c10::optional<at::Tensor>& lam = c10::nullopt);
// The LARS block of a fused SGD step (csrc/kernels/lars.h): descriptor, meta and partials from
// lars_plan, the partials filled by lars_norms just before; ratios: one float per parameter.
// Without a descriptor the step is plain SGD.
struct LarsStep {
  c10::optional<at::Tensor> desc, meta, part, ratios;
  double trust_coefficient = 0.0, eps = 0.0;
  bool exclude = true;
};
std::vector<at::Tensor> lars_plan(const at::Tensor& flat, int64_t s, int64_t e, const std::vector<int64_t>& offsets,
                                  const std::vector<int64_t>& numels, const std::vector<int64_t>& ndims,
                                  const std::vector<int64_t>& slots,
                                  const c10::optional<at::Tensor>& prep_desc = c10::nullopt,
                                  const c10::optional<at::Tensor>& prep_meta = c10::nullopt);
void lars_norms(const at::Tensor& w, const at::Tensor& g, const at::Tensor& desc, const at::Tensor& meta, at::Tensor part);
int64_t lars_chunk_(int64_t n);   // floats per norms chunk of a parameter of n floats
int64_t lars_nparts_(int64_t n);  // chunks (= partial pairs) of such a parameter
std::vector<at::Tensor> sgd_prep_plan(const at::Tensor& flat, int64_t s, int64_t e, const std::vector<at::Tensor>& ws,
                                      const std::vector<bool>& want_t,
                                      const c10::optional<at::Tensor>& amax_out = c10::nullopt,
                                      const std::vector<int64_t>& amax_offsets = {},
                                      const std::vector<int64_t>& cuts = {});
void sgd_step_prep(at::Tensor p, const at::Tensor& g, c10::optional<at::Tensor> buf, const c10::optional<at::Tensor>& lr_t,
                   double lr, double momentum, double dampening, double wd, double grad_scale, bool nesterov, bool first,
                   bool maximize, const at::Tensor& desc, const at::Tensor& meta, at::Tensor amax,
                   const c10::optional<at::Tensor>& counter, const c10::optional<at::Tensor>& clip_part = c10::nullopt,
                   double max_norm = 0.0, const c10::optional<at::Tensor>& stats = c10::nullopt,
                   bool skip_nonfinite = false, const LarsStep& lars = LarsStep{},
                   const c10::optional<at::Tensor>& ema = c10::nullopt,
                   const c10::optional<at::Tensor>& ema_coef = c10::nullopt,
                   const c10::optional<at::Tensor>& sched_state = c10::nullopt,
                   const c10::optional<at::Tensor>& sched_cfg = c10::nullopt,
                   const c10::optional<at::Tensor>& sched_last = c10::nullopt, bool sched_advance = false);
void sgd_step(at::Tensor p, const at::Tensor& g, c10::optional<at::Tensor> buf, const c10::optional<at::Tensor>& lr_t,
              double lr, double momentum, double dampening, double wd, double grad_scale, bool nesterov, bool first,
              bool maximize, const c10::optional<at::Tensor>& counter,
              const c10::optional<at::Tensor>& clip_part = c10::nullopt, double max_norm = 0.0,
              const c10::optional<at::Tensor>& stats = c10::nullopt, bool skip_nonfinite = false,
              const LarsStep& lars = LarsStep{}, const c10::optional<at::Tensor>& ema = c10::nullopt,
              const c10::optional<at::Tensor>& ema_coef = c10::nullopt,
              const c10::optional<at::Tensor>& sched_state = c10::nullopt,
              const c10::optional<at::Tensor>& sched_cfg = c10::nullopt,
              const c10::optional<at::Tensor>& sched_last = c10::nullopt, bool sched_advance = false);
// AdamW / LAMB over a flat range (csrc/kernels/adam.h). The LAMB block: descriptor, meta and partials from
// lars_plan, the partials filled by lamb_moments just before; ratios: one float per parameter. Without a
// descriptor the step is AdamW.
struct LambStep {
  c10::optional<at::Tensor> desc, meta, part, ratios;
  bool exclude = true;
};
// One step over w, g, m (exp_avg), v (exp_avg_sq), flat and of one size. state = {t, arrivals} (int64,
// device): every workgroup reads t; with advance (the last launch of a step()) the launch stores t + 1.
// The clip, EMA and schedule blocks are sgd_step's.
void adam_step(at::Tensor w, const at::Tensor& g, at::Tensor m, at::Tensor v, const c10::optional<at::Tensor>& lr_t,
               double lr, double beta1, double beta2, double eps, double wd, bool maximize, at::Tensor state,
               bool advance, const c10::optional<at::Tensor>& counter = c10::nullopt,
               const c10::optional<at::Tensor>& clip_part = c10::nullopt, double max_norm = 0.0,
               const c10::optional<at::Tensor>& stats = c10::nullopt, bool skip_nonfinite = false,
               const LambStep& lamb = LambStep{}, const c10::optional<at::Tensor>& ema = c10::nullopt,
               const c10::optional<at::Tensor>& ema_coef = c10::nullopt,
               const c10::optional<at::Tensor>& sched_state = c10::nullopt,
               const c10::optional<at::Tensor>& sched_cfg = c10::nullopt,
               const c10::optional<at::Tensor>& sched_last = c10::nullopt, bool sched_advance = false);
// LAMB pass 1: the new m, v and the fp64 pairs {sum w^2, sum r^2} of lamb's work list (reads t only)
void lamb_moments(const at::Tensor& w, const at::Tensor& g, at::Tensor m, at::Tensor v, double beta1, double beta2,
                  double eps, double wd, bool maximize, const at::Tensor& state, const LambStep& lamb,
                  const c10::optional<at::Tensor>& clip_part = c10::nullopt, double max_norm = 0.0,
                  bool skip_nonfinite = false);
int64_t adam_grid_(int64_t n);  // workgroups of the flat adam_step launch over n floats (without LAMB)
// Learning-rate schedule of the fused step (csrc/kernels/lr_sched.h). sched_state = {t, arrivals} (int64,
// device), sched_cfg = lr_sched_pack's bytes moved to the device, sched_last = one float32 that receives the
// rate of the launch (optional); sched_advance: this launch is the last of its step() and stores t + 1.
// lr_sched_pack: the configuration as CPU bytes (kind: 0 constant, 1 cosine, 2 poly, 3 step).
at::Tensor lr_sched_pack(int64_t kind, int64_t warmup_steps, double warmup_start_factor, int64_t total_steps,
                         double end_factor, double power, const std::vector<int64_t>& milestones, double gamma);
// float32 [n]: the rates of steps first .. first + n - 1 for the base rate (lr_t ? lr_t[0] : lr)
at::Tensor lr_sched_table(const at::Tensor& cfg, const c10::optional<at::Tensor>& lr_t, double lr, int64_t first,
                          int64_t n);
// one step of the schedule without an SGD launch: last = rate of step t, t += 1, arrivals = 0
void lr_sched_advance(at::Tensor state, const at::Tensor& cfg, const c10::optional<at::Tensor>& last,
                      const c10::optional<at::Tensor>& lr_t, double lr);
int64_t sgd_grid_(int64_t n);  // workgroups of the flat sgd_step launch over n floats
// gradient-norm clipping over a flat fp32 range (csrc/kernels/grad_norm.hip): part[0 .. grad_norm_parts(n))
// fp64 partial sums of squares; clip_scale: g *= min(max_norm / (norm + 1e-6), 1), stats = {norm, coef, -}
int64_t grad_norm_parts_(int64_t n);
int64_t grad_norm_chunk_(int64_t n);
void grad_sumsq(const at::Tensor& g, at::Tensor part);
void clip_scale(at::Tensor g, const at::Tensor& part, double max_norm, const c10::optional<at::Tensor>& stats);
at::Tensor augment(const at::Tensor& images, const c10::optional<at::Tensor>& indices, int64_t idx_offset, int64_t batch,
                   std::vector<double> mean, std::vector<double> std_, int64_t pad, bool flip,
                   const c10::optional<at::Tensor>& counter, int64_t seed, c10::optional<at::Tensor> out,
                   int64_t nbatches = 0, const c10::optional<at::Tensor>& labels = c10::nullopt,
                   const c10::optional<at::Tensor>& labels_out = c10::nullopt, double mixup_alpha = 0.0,
                   double cutmix_alpha = 0.0, double mix_prob = 1.0, double mix_switch_prob = 0.5,
                   const c10::optional<at::Tensor>& mix = c10::nullopt,
                   const c10::optional<at::Tensor>& labels_b = c10::nullopt, double erase_prob = 0.0,
                   std::vector<double> erase_scale = {0.02, 0.33}, std::vector<double> erase_ratio = {0.3, 3.3},
                   const std::string& erase_mode = "const", std::vector<double> erase_value = {0.0},
                   const c10::optional<at::Tensor>& erase = c10::nullopt);
// float32 [n, 8]: the rows {mode, lam, lam_raw, y0, y1, x0, x1, 0} augment publishes at counters first_counter + i
at::Tensor mix_params(int64_t seed, int64_t first_counter, int64_t n, double mixup_alpha, double cutmix_alpha,
                      double mix_prob, double mix_switch_prob, int64_t H, int64_t W);
// The augment launch with a resize (3-channel images): RandomResizedCrop (train; scale and ratio are (lo, hi) pairs)
// or the central window of fraction center_frac, resampled bilinearly to out_h x out_w, then flip / normalise /
// mix / erase as augment (the erase box in output pixels). crops: int32 [batch, 5], receives {top, left, h, w, flip}
// per image.
at::Tensor augment_resize(const at::Tensor& images, const c10::optional<at::Tensor>& indices, int64_t idx_offset,
                          int64_t batch, std::vector<double> mean, std::vector<double> std_, int64_t out_h,
                          int64_t out_w, bool train, std::vector<double> scale, std::vector<double> ratio,
                          double center_frac, bool flip, const c10::optional<at::Tensor>& counter, int64_t seed,
                          c10::optional<at::Tensor> out, int64_t nbatches, const c10::optional<at::Tensor>& labels,
                          const c10::optional<at::Tensor>& labels_out, const at::Tensor& crops,
                          double mixup_alpha = 0.0, double cutmix_alpha = 0.0, double mix_prob = 1.0,
                          double mix_switch_prob = 0.5, const c10::optional<at::Tensor>& mix = c10::nullopt,
                          const c10::optional<at::Tensor>& labels_b = c10::nullopt, double erase_prob = 0.0,
                          std::vector<double> erase_scale = {0.02, 0.33}, std::vector<double> erase_ratio = {0.3, 3.3},
                          const std::string& erase_mode = "const", std::vector<double> erase_value = {0.0},
                          const c10::optional<at::Tensor>& erase = c10::nullopt);
// int32 [n, B, 4]: the windows {top, left, h, w} augment_resize draws at counters first_counter + i for image slot b
at::Tensor rrc_params(int64_t seed, int64_t first_counter, int64_t n, int64_t B, std::vector<double> scale,
                      std::vector<double> ratio, int64_t H, int64_t W);
// int32 [n, B, 5]: the rows {on, top, left, h, w} the augment launches publish at counters first_counter + i for
// image slot b of an H x W output (RandomErasing, erase_prob = prob)
at::Tensor erase_params(int64_t seed, int64_t first_counter, int64_t n, int64_t B, double prob,
                        std::vector<double> scale, std::vector<double> ratio, int64_t H, int64_t W);
// float32 [B, 3, H, W] channels_last: the N(0, 1) fill noise of the erase modes rand and pixel at one counter
at::Tensor erase_noise(int64_t seed, int64_t counter, int64_t B, int64_t H, int64_t W);
// RandAugment (randaug.h): stage `batch` images as uint8 [batch, out_h, out_w, 3] into buf_a (the gather of augment;
// resize: RandomResizedCrop with integer bilinear taps, crops receives {top, left, h, w, flip}; otherwise the
// pad-shift crop) and apply num_ops drawn operations per image ping-pong between buf_a and buf_b: the result is in
// buf_a for an even num_ops, in buf_b for an odd one. ops: op kinds to draw from; fill: three ints in 0 .. 255;
// rows: int32 [batch, num_ops, 8], receives the rows. One launch.
void randaug(const at::Tensor& images, const c10::optional<at::Tensor>& indices, int64_t idx_offset, int64_t batch,
             int64_t out_h, int64_t out_w, bool resize, std::vector<double> scale, std::vector<double> ratio,
             int64_t pad, bool flip, const c10::optional<at::Tensor>& counter, int64_t seed, int64_t nbatches,
             const at::Tensor& labels, at::Tensor labels_out, const c10::optional<at::Tensor>& crops, int64_t num_ops,
             double magnitude, double mstd, std::vector<int64_t> ops, std::vector<int64_t> fill, at::Tensor buf_a,
             at::Tensor buf_b, at::Tensor rows);
// int32 [n, B, num_ops, 8]: the rows randaug publishes at counters first_counter + i for an H x W staged image
at::Tensor randaug_params(int64_t seed, int64_t first_counter, int64_t n, int64_t B, int64_t num_ops, double magnitude,
                          double mstd, std::vector<int64_t> ops, std::vector<int64_t> fill, int64_t H, int64_t W);
// Stochastic depth (drop_path.h). rates: device fp32 [nb], one drop probability in [0, 1) per block.
// float32 [nb, B]: the scales of step counter[0] (a device int64 tensor), which the launch then advances by one
at::Tensor drop_path_draw(at::Tensor counter, int64_t seed, const at::Tensor& rates, int64_t B);
// float32 [n, nb, B]: the tables drop_path_draw writes at step counters first .. first + n - 1
at::Tensor drop_path_table(int64_t seed, int64_t first, int64_t n, const at::Tensor& rates, int64_t B);
void counter_inc(at::Tensor c);
void stack_mean(const std::vector<at::Tensor>& srcs, at::Tensor dst);
void gpu_sleep(double us);
void gpu_timestamp(at::Tensor ts, int64_t idx);
int64_t gpu_wall_clock_khz();
void scale_(at::Tensor x, double a);
std::vector<at::Tensor> maxpool2d_fwd(const at::Tensor& x, int64_t k, int64_t s, int64_t p);
at::Tensor maxpool2d_bwd(const at::Tensor& gy, const at::Tensor& arg, std::vector<int64_t> in_shape, int64_t k,
                         int64_t s, int64_t p);
at::Tensor avgpool_fwd(const at::Tensor& x);
at::Tensor avgpool_bwd(const at::Tensor& gy, std::vector<int64_t> in_shape);

// CDP_GEMM_LOG=1: the GEMM launches so far as (kind, M, N, K, bm, bn, splits), in enqueue order
std::vector<std::tuple<std::string, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>> gemm_log(bool clear);

}  // namespace cdp
