// Python bindings of the native runtime: kernels (ops.cpp), RCCL communicator, bucketed reducer.
#include <torch/csrc/utils/pybind.h>
#include <torch/extension.h>

#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include "ops.h"
#include "rccl_comm.h"
#include "reducer.h"

namespace py = pybind11;
using namespace cdp;

namespace {
// Diagnostics (CDP_SEGV_BT=1 at import): print the native stack of a SIGSEGV to stderr, then die
// with the default action. Host-side only; no debugger attaches to the GPU process.
void segv_backtrace(int sig) {
  void* frames[64];
  const int n = backtrace(frames, 64);
  const char msg[] = "[cdp] native backtrace:\n";
  (void)!write(2, msg, sizeof(msg) - 1);
  backtrace_symbols_fd(frames, n, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}
}  // namespace

PYBIND11_MODULE(_C, m) {
  if (const char* bt = std::getenv("CDP_SEGV_BT"); bt && bt[0] == '1') signal(SIGSEGV, segv_backtrace);
  m.doc() = "cs744_distributed_data_parallel_amd native runtime (gfx950 kernels, RCCL comm, reducer)";
  m.attr("ARCH") = "gfx950";

  // -------------------------------------------------------------- kernels
  m.def("set_conv_gemm", &set_conv_gemm, py::arg("mode"),
        "select the conv GEMM engine: x3 (3-term bf16 split), f16x2 (scaled 2-term fp16 split), f32 (exact fp32 "
        "MFMA) or bf16 (bf16 operands, non-parity)");
  m.def("get_conv_gemm", &get_conv_gemm);
  m.def("set_gemm_override", &set_gemm_override, py::arg("kind"), py::arg("bm") = 0, py::arg("bn") = 0,
        py::arg("splits") = 0, "force the tile / split-K plan of later GEMMs (tuning sweeps; zeros restore the planner)");
  m.def("pair_launches", &pair_launches, "paired data/weight-gradient launches issued so far");
  m.def("plan_info", &plan_info, py::arg("kind"), py::arg("M"), py::arg("N"), py::arg("K"));
  m.def("clear_hip_error", [] { return std::string(hipGetErrorName(hipGetLastError())); },
        "reset the thread's last HIP error (e.g. after an invalidated stream capture) and return its name");
  m.def("conv2d_fwd", &conv2d_fwd, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("stride"), py::arg("pad"),
        py::arg("want_stats") = false, py::arg("x_amax") = py::none(), py::arg("w_amax") = py::none());
  m.def("conv2d_dgrad", &conv2d_dgrad, py::arg("dy"), py::arg("w"), py::arg("in_shape"), py::arg("stride"),
        py::arg("pad"), py::arg("addend") = py::none(), py::arg("dy_amax") = py::none(), py::arg("w_amax") = py::none(),
        py::arg("w_t") = py::none());
  m.def("conv2d_wgrad", &conv2d_wgrad, py::arg("dy"), py::arg("x"), py::arg("w_shape"), py::arg("stride"),
        py::arg("pad"), py::arg("out") = py::none(), py::arg("accumulate") = false, py::arg("dy_amax") = py::none(),
        py::arg("x_amax") = py::none());
  m.def("conv_bn_act_fwd", &conv_bn_act_fwd, py::arg("x"), py::arg("w"), py::arg("b"), py::arg("gamma"),
        py::arg("beta"), py::arg("running_mean"), py::arg("running_var"), py::arg("num_batches_tracked"),
        py::arg("momentum"), py::arg("eps"), py::arg("training"), py::arg("stride"), py::arg("pad"), py::arg("pool"),
        py::arg("relu"), py::arg("residual"), py::arg("x_amax") = py::none(), py::arg("w_amax") = py::none(),
        py::arg("res_y") = py::none(), py::arg("res_stats") = py::none(), py::arg("defer_apply") = false,
        py::arg("drop_scale") = py::none(),
        "fused conv + BN [+ residual] [+ ReLU] [+ 2x2 max-pool] forward; returns (out, y, stats, x_saved, out_amax, "
        "x_amax, w_amax, relu_mask). defer_apply: statistics only, out a shape-only placeholder; res_y / res_stats: "
        "the residual as such a deferred branch's raw output and stats, normalized inside this block's apply pass; "
        "drop_scale (residual blocks): fp32 [N], the BN output of image b is multiplied by drop_scale[b] before the add");
  m.def("act_max", &act_max_of, py::arg("t"),
        "f16x2 engine: an activation's per-image / per-channel |max| slots by the standalone pass (int32 [N + "
        "copies * C], float bits; undefined tensor for other engines)");
  m.def("act_max_memsets", &act_max_memsets, "slot-chunk memsets issued so far (tests)");
  m.def("act_max_copies", &act_max_copies, "per-channel slot copies of an act max");
  m.def("conv_bn_act_bwd", &conv_bn_act_bwd, py::arg("gout"), py::arg("x"), py::arg("w"), py::arg("y"),
        py::arg("stats"), py::arg("stride"), py::arg("pad"), py::arg("pool"), py::arg("relu"), py::arg("need_dx"),
        py::arg("has_bias"), py::arg("zout") = py::none(), py::arg("training") = true, py::arg("dw_out") = py::none(),
        py::arg("db_out") = py::none(), py::arg("dgamma_out") = py::none(), py::arg("dbeta_out") = py::none(),
        py::arg("dx_addend") = py::none(), py::arg("x_amax") = py::none(), py::arg("w_amax") = py::none(),
        py::arg("w_t") = py::none(), py::arg("part_in") = py::none(), py::arg("prev_y") = py::none(),
        py::arg("prev_stats") = py::none(), py::arg("prev_pool") = false, py::arg("prev_relu") = false,
        py::arg("prev_ps") = 2, py::arg("bias") = py::none(), py::arg("drop_scale") = py::none(),
        "fused block backward; returns (dx, dw, db, dgamma, dbeta, dres, prev_part, dy_amax). prev_* describe the BN whose "
        "output is x: its statistics reduction is then fused into this block's data-gradient reduction and returned "
        "as prev_part (undefined when not fused), which that block's backward takes as part_in");
  m.def("weight_prep_into", &weight_prep_into, py::arg("weights"), py::arg("want_t"), py::arg("amax"), py::arg("wts"),
        "weight_prep writing into existing buffers (a fused-step plan's)");
  m.def("weight_prep", &weight_prep, py::arg("weights"), py::arg("want_t"),
        "one launch per step: conv weights' |max| partials (f16x2; else empty) and W^T [Ci, KH*KW*Co] per weight "
        "with want_t (the data-gradient operand)");
  m.def("linear_fwd", &linear_fwd);
  m.def("linear_bwd", &linear_bwd, py::arg("gy"), py::arg("x"), py::arg("w"), py::arg("need_dx"),
        py::arg("has_bias"), py::arg("dw_out") = py::none(), py::arg("db_out") = py::none());
  m.def("xent_fwd", &xent_fwd, py::arg("logits"), py::arg("target"), py::arg("correct") = py::none(),
        py::arg("label_smoothing") = 0.0, py::arg("topk") = 1, py::arg("target_b") = py::none(),
        py::arg("lam") = py::none());
  m.def("xent_bwd", &xent_bwd, py::arg("gloss"), py::arg("logits"), py::arg("target"), py::arg("label_smoothing") = 0.0,
        py::arg("target_b") = py::none(), py::arg("lam") = py::none());
  m.def("bce_fwd", &bce_fwd, py::arg("logits"), py::arg("target"), py::arg("label_smoothing") = 0.0,
        py::arg("target_threshold") = py::none(), py::arg("sum_classes") = false, py::arg("target_b") = py::none(),
        py::arg("lam") = py::none(),
        "binary cross-entropy with logits against the smoothed, mixed, optionally thresholded one-hot rows");
  m.def("bce_bwd", &bce_bwd, py::arg("gloss"), py::arg("logits"), py::arg("target"), py::arg("label_smoothing") = 0.0,
        py::arg("target_threshold") = py::none(), py::arg("sum_classes") = false, py::arg("target_b") = py::none(),
        py::arg("lam") = py::none());
  m.def("gemm_log", &gemm_log, py::arg("clear") = false,
        "CDP_GEMM_LOG=1: (kind, M, N, K, bm, bn, splits) of every conv / weight-gradient GEMM launch so far");
  m.def("xent_linear_bwd", &xent_linear_bwd, py::arg("gloss"), py::arg("logits"), py::arg("target"), py::arg("x"),
        py::arg("w"), py::arg("need_dx"), py::arg("has_bias"), py::arg("dw_out") = py::none(),
        py::arg("db_out") = py::none(), py::arg("link_y") = py::none(), py::arg("link_stats") = py::none(),
        py::arg("link_pool") = false, py::arg("link_relu") = false, py::arg("link_ps") = 2,
        py::arg("label_smoothing") = 0.0, py::arg("target_b") = py::none(), py::arg("lam") = py::none(),
        py::arg("bce") = false, py::arg("target_threshold") = py::none(), py::arg("sum_classes") = false,
        "CrossEntropy (bce: binary cross-entropy) backward + narrow Linear backward in one launch (+ the BN backward partials of the block "
        "that produced the Linear's input, link_*): {dlogits, dx, dw, db, part}");
  py::class_<LarsStep>(m, "LarsStep", "the LARS block of sgd_step / sgd_step_prep (default: off)")
      .def(py::init([](c10::optional<at::Tensor> desc, c10::optional<at::Tensor> meta, c10::optional<at::Tensor> part,
                       c10::optional<at::Tensor> ratios, double trust_coefficient, double eps, bool exclude) {
             LarsStep l;
             l.desc = desc, l.meta = meta, l.part = part, l.ratios = ratios;
             l.trust_coefficient = trust_coefficient, l.eps = eps, l.exclude = exclude;
             return l;
           }),
           py::arg("desc") = py::none(), py::arg("meta") = py::none(), py::arg("part") = py::none(),
           py::arg("ratios") = py::none(), py::arg("trust_coefficient") = 0.0, py::arg("eps") = 0.0,
           py::arg("exclude") = true);
  m.def("lars_plan", &lars_plan, py::arg("flat"), py::arg("start"), py::arg("end"), py::arg("offsets"),
        py::arg("numels"), py::arg("ndims"), py::arg("slots"), py::arg("prep_desc") = py::none(),
        py::arg("prep_meta") = py::none(),
        "plan of the LARS norms pass and step over an arena range: {descriptor, meta, fp64 partial pairs}");
  m.def("lars_norms", &lars_norms, py::arg("w"), py::arg("g"), py::arg("desc"), py::arg("meta"), py::arg("part"),
        "per-parameter fp64 partial sums of squares {w^2, g^2} of an arena range (every pair is written)");
  m.def("lars_chunk", &lars_chunk_, py::arg("n"), "floats per norms chunk of a parameter of n floats");
  m.def("lars_nparts", &lars_nparts_, py::arg("n"), "norms chunks of a parameter of n floats");
  m.def("sgd_step", &sgd_step, py::arg("p"), py::arg("g"), py::arg("buf"), py::arg("lr_t"), py::arg("lr"),
        py::arg("momentum"), py::arg("dampening"), py::arg("wd"), py::arg("grad_scale"), py::arg("nesterov"),
        py::arg("first"), py::arg("maximize"), py::arg("counter") = py::none(), py::arg("clip_part") = py::none(),
        py::arg("max_norm") = 0.0, py::arg("stats") = py::none(), py::arg("skip_nonfinite") = false,
        py::arg("lars") = LarsStep{}, py::arg("ema") = py::none(), py::arg("ema_coef") = py::none(),
        py::arg("sched_state") = py::none(), py::arg("sched_cfg") = py::none(), py::arg("sched_last") = py::none(),
        py::arg("sched_advance") = false);
  py::class_<LambStep>(m, "LambStep", "the LAMB block of adam_step / lamb_moments (default: off, AdamW)")
      .def(py::init([](c10::optional<at::Tensor> desc, c10::optional<at::Tensor> meta, c10::optional<at::Tensor> part,
                       c10::optional<at::Tensor> ratios, bool exclude) {
             LambStep l;
             l.desc = desc, l.meta = meta, l.part = part, l.ratios = ratios, l.exclude = exclude;
             return l;
           }),
           py::arg("desc") = py::none(), py::arg("meta") = py::none(), py::arg("part") = py::none(),
           py::arg("ratios") = py::none(), py::arg("exclude") = true);
  m.def("adam_step", &adam_step, py::arg("w"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("lr_t"), py::arg("lr"),
        py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("wd"), py::arg("maximize"), py::arg("state"),
        py::arg("advance"), py::arg("counter") = py::none(), py::arg("clip_part") = py::none(),
        py::arg("max_norm") = 0.0, py::arg("stats") = py::none(), py::arg("skip_nonfinite") = false,
        py::arg("lamb") = LambStep{}, py::arg("ema") = py::none(), py::arg("ema_coef") = py::none(),
        py::arg("sched_state") = py::none(), py::arg("sched_cfg") = py::none(), py::arg("sched_last") = py::none(),
        py::arg("sched_advance") = false,
        "AdamW (or, with a LAMB block, LAMB's pass 2) over a flat range; state = {t, arrivals} on the device");
  m.def("lamb_moments", &lamb_moments, py::arg("w"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("wd"), py::arg("maximize"), py::arg("state"), py::arg("lamb"),
        py::arg("clip_part") = py::none(), py::arg("max_norm") = 0.0, py::arg("skip_nonfinite") = false,
        "LAMB pass 1: the new exp_avg / exp_avg_sq and the fp64 pairs {sum w^2, sum r^2} of every work item");
  m.def("adam_grid", &adam_grid_, py::arg("n"), "workgroups of the flat adam_step launch over n floats");
  m.def("lr_sched_pack", &lr_sched_pack, py::arg("kind"), py::arg("warmup_steps"), py::arg("warmup_start_factor"),
        py::arg("total_steps"), py::arg("end_factor"), py::arg("power"), py::arg("milestones"), py::arg("gamma"),
        "the learning-rate schedule's configuration as CPU bytes (kind: 0 constant, 1 cosine, 2 poly, 3 step)");
  m.def("lr_sched_table", &lr_sched_table, py::arg("cfg"), py::arg("lr_t"), py::arg("lr"), py::arg("first"),
        py::arg("n"), "float32 [n]: the rates the fused step uses at schedule steps first .. first + n - 1");
  m.def("lr_sched_advance", &lr_sched_advance, py::arg("state"), py::arg("cfg"), py::arg("last") = py::none(),
        py::arg("lr_t") = py::none(), py::arg("lr") = 0.0,
        "one step of the schedule without an SGD launch (a step() that launches nothing)");
  m.def("sgd_grid", &sgd_grid_, py::arg("n"), "workgroups of the flat sgd_step launch over n floats");
  m.def("grad_norm_parts", &grad_norm_parts_, py::arg("n"), "partials grad_sumsq writes for a range of n floats");
  m.def("grad_norm_chunk", &grad_norm_chunk_, py::arg("n"), "floats of the range each grad_sumsq workgroup owns");
  m.def("grad_sumsq", &grad_sumsq, py::arg("g"), py::arg("part"),
        "fp64 partial sums of squares of a flat fp32 range (all grad_norm_parts(n) partials are written)");
  m.def("clip_scale", &clip_scale, py::arg("g"), py::arg("part"), py::arg("max_norm"), py::arg("stats") = py::none(),
        "g *= min(max_norm / (norm + 1e-6), 1) in place from grad_sumsq's partials; stats[0..1] = norm, coef");
  m.def("sgd_prep_plan", &sgd_prep_plan, py::arg("flat"), py::arg("start"), py::arg("end"), py::arg("weights"),
        py::arg("want_t"), py::arg("amax_out") = py::none(), py::arg("amax_offsets") = std::vector<int64_t>{},
        py::arg("cuts") = std::vector<int64_t>{},
        "plan of the fused SGD + weight-preparation step over an arena range");
  m.def("sgd_step_prep", &sgd_step_prep, py::arg("p"), py::arg("g"), py::arg("buf"), py::arg("lr_t"), py::arg("lr"),
        py::arg("momentum"), py::arg("dampening"), py::arg("wd"), py::arg("grad_scale"), py::arg("nesterov"),
        py::arg("first"), py::arg("maximize"), py::arg("desc"), py::arg("meta"), py::arg("amax"),
        py::arg("counter") = py::none(), py::arg("clip_part") = py::none(), py::arg("max_norm") = 0.0,
        py::arg("stats") = py::none(), py::arg("skip_nonfinite") = false, py::arg("lars") = LarsStep{},
        py::arg("ema") = py::none(), py::arg("ema_coef") = py::none(), py::arg("sched_state") = py::none(),
        py::arg("sched_cfg") = py::none(), py::arg("sched_last") = py::none(), py::arg("sched_advance") = false,
        "SGD over an arena range that also emits the next step's weight |max| / W^T");
  m.def("augment", &augment, py::arg("images"), py::arg("indices"), py::arg("idx_offset"), py::arg("batch"),
        py::arg("mean"), py::arg("std"), py::arg("pad"), py::arg("flip"), py::arg("counter"), py::arg("seed"),
        py::arg("out") = py::none(), py::arg("nbatches") = 0, py::arg("labels") = py::none(),
        py::arg("labels_out") = py::none(), py::arg("mixup_alpha") = 0.0, py::arg("cutmix_alpha") = 0.0,
        py::arg("mix_prob") = 1.0, py::arg("mix_switch_prob") = 0.5, py::arg("mix") = py::none(),
        py::arg("labels_b") = py::none(), py::arg("erase_prob") = 0.0,
        py::arg("erase_scale") = std::vector<double>{0.02, 0.33},
        py::arg("erase_ratio") = std::vector<double>{0.3, 3.3}, py::arg("erase_mode") = "const",
        py::arg("erase_value") = std::vector<double>{0.0}, py::arg("erase") = py::none(),
        "gather + RandomCrop + flip + normalize one batch (NHWC fp32); nbatches > 0 takes the batch offset from "
        "the step counter; labels_out receives the batch's labels; an alpha > 0 mixes image b with image "
        "batch - 1 - b (mixup / CutMix), publishing {mode, lam, lam_raw, y0, y1, x0, x1, 0} in mix and the "
        "partners' labels in labels_b; erase_prob > 0 erases a box of every image with that probability before "
        "the mix (RandomErasing; mode const / rand / pixel), publishing {on, top, left, h, w} per image in erase "
        "(int32 [batch, 5])");
  m.def("mix_params", &mix_params, py::arg("seed"), py::arg("first_counter"), py::arg("n"),
        py::arg("mixup_alpha") = 0.0, py::arg("cutmix_alpha") = 0.0, py::arg("mix_prob") = 1.0,
        py::arg("mix_switch_prob") = 0.5, py::arg("H") = 32, py::arg("W") = 32,
        "float32 [n, 8]: the mix rows augment publishes at step counters first_counter .. first_counter + n - 1");
  m.def("augment_resize", &augment_resize, py::arg("images"), py::arg("indices"), py::arg("idx_offset"),
        py::arg("batch"), py::arg("mean"), py::arg("std"), py::arg("out_h"), py::arg("out_w"), py::arg("train"),
        py::arg("scale"), py::arg("ratio"), py::arg("center_frac"), py::arg("flip"), py::arg("counter"),
        py::arg("seed"), py::arg("out") = py::none(), py::arg("nbatches") = 0, py::arg("labels") = py::none(),
        py::arg("labels_out") = py::none(), py::arg("crops"), py::arg("mixup_alpha") = 0.0,
        py::arg("cutmix_alpha") = 0.0, py::arg("mix_prob") = 1.0, py::arg("mix_switch_prob") = 0.5,
        py::arg("mix") = py::none(), py::arg("labels_b") = py::none(), py::arg("erase_prob") = 0.0,
        py::arg("erase_scale") = std::vector<double>{0.02, 0.33},
        py::arg("erase_ratio") = std::vector<double>{0.3, 3.3}, py::arg("erase_mode") = "const",
        py::arg("erase_value") = std::vector<double>{0.0}, py::arg("erase") = py::none(),
        "gather + RandomResizedCrop (train) or central crop of center_frac + bilinear resize to out_h x out_w + "
        "flip + normalize one batch (NHWC fp32, 3 channels); crops (int32 [batch, 5]) receives {top, left, h, w, "
        "flip} per image; idx, nbatches, labels, the mix and the erase arguments as augment (the CutMix and erase boxes "
        "in output pixels)");
  m.def("rrc_params", &rrc_params, py::arg("seed"), py::arg("first_counter"), py::arg("n"), py::arg("B"),
        py::arg("scale"), py::arg("ratio"), py::arg("H"), py::arg("W"),
        "int32 [n, B, 4]: the windows {top, left, h, w} augment_resize draws at step counters first_counter .. "
        "first_counter + n - 1");
  m.def("erase_params", &erase_params, py::arg("seed"), py::arg("first_counter"), py::arg("n"), py::arg("B"),
        py::arg("prob"), py::arg("scale"), py::arg("ratio"), py::arg("H"), py::arg("W"),
        "int32 [n, B, 5]: the erase rows {on, top, left, h, w} augment / augment_resize publish at step counters "
        "first_counter .. first_counter + n - 1 for an H x W output");
  m.def("erase_noise", &erase_noise, py::arg("seed"), py::arg("counter"), py::arg("B"), py::arg("H"), py::arg("W"),
        "float32 [B, 3, H, W] channels_last: the N(0, 1) fill noise of the erase modes rand and pixel at one "
        "step counter");
  m.def("randaug", &randaug, py::arg("images"), py::arg("indices"), py::arg("idx_offset"), py::arg("batch"),
        py::arg("out_h"), py::arg("out_w"), py::arg("resize"), py::arg("scale"), py::arg("ratio"), py::arg("pad"),
        py::arg("flip"), py::arg("counter"), py::arg("seed"), py::arg("nbatches"), py::arg("labels"),
        py::arg("labels_out"), py::arg("crops"), py::arg("num_ops"), py::arg("magnitude"), py::arg("mstd"),
        py::arg("ops"), py::arg("fill"), py::arg("buf_a"), py::arg("buf_b"), py::arg("rows"),
        "RandAugment: gather + crop (pad-shift, or RandomResizedCrop with an exact integer bilinear resize) + flip one "
        "batch as uint8 [batch, out_h, out_w, 3] and apply num_ops drawn operations per image in one launch; the "
        "result is in buf_a for an even num_ops and in buf_b for an odd one; rows (int32 [batch, num_ops, 8]) "
        "receives {op | sign << 8, level_q, p0 .. p5} per operation");
  m.def("randaug_params", &randaug_params, py::arg("seed"), py::arg("first_counter"), py::arg("n"), py::arg("B"),
        py::arg("num_ops"), py::arg("magnitude"), py::arg("mstd"), py::arg("ops"), py::arg("fill"), py::arg("H"),
        py::arg("W"),
        "int32 [n, B, num_ops, 8]: the rows randaug publishes at step counters first_counter .. first_counter + n - 1 "
        "for an H x W staged image");
  m.def("drop_path_draw", &drop_path_draw, py::arg("counter"), py::arg("seed"), py::arg("rates"), py::arg("B"),
        "float32 [nb, B]: the stochastic-depth scales (0 or 1 / (1 - rates[i])) of step counter[0] for nb blocks and "
        "B images, in one launch that then advances the device int64 counter by one");
  m.def("drop_path_table", &drop_path_table, py::arg("seed"), py::arg("first"), py::arg("n"), py::arg("rates"),
        py::arg("B"),
        "float32 [n, nb, B]: the tables drop_path_draw writes at step counters first .. first + n - 1 (no counter moves)");
  m.def("counter_inc", &counter_inc);
  m.def("stack_mean", &stack_mean);
  m.def("scale_", &scale_);
  m.def("gpu_sleep", &gpu_sleep, py::arg("us"), "idle one workgroup ~us on the current stream");
  m.def("gpu_wall_clock_khz", &gpu_wall_clock_khz);
  m.def("gpu_timestamp", &gpu_timestamp, py::arg("ts"), py::arg("idx"), "ts[idx] = GPU wall clock (100 MHz)");
  m.def("create_stream",
        [](int priority, bool nonblocking, bool cu_mask) {
          hipStream_t st = nullptr;
          if (cu_mask) {
            uint32_t mask[8];
            for (auto& w : mask) w = 0xffffffffu;  // every CU: a stream on a queue of its own
            TORCH_CHECK(hipExtStreamCreateWithCUMask(&st, 8, mask) == hipSuccess, "hipExtStreamCreateWithCUMask failed");
          } else {
            TORCH_CHECK(hipStreamCreateWithPriority(&st, nonblocking ? hipStreamNonBlocking : hipStreamDefault,
                                                    priority) == hipSuccess,
                        "hipStreamCreateWithPriority failed");
          }
          return reinterpret_cast<intptr_t>(st);
        },
        py::arg("priority") = 0, py::arg("nonblocking") = true, py::arg("cu_mask") = false,
        "diagnostics: a raw HIP stream for torch.cuda.ExternalStream; the caller destroys it with "
        "destroy_stream before the process exits (HIP's own teardown must not meet a live CU-masked queue)");
  m.def("destroy_stream", [](intptr_t s) {
    hipStream_t st = reinterpret_cast<hipStream_t>(s);
    TORCH_CHECK(hipStreamSynchronize(st) == hipSuccess && hipStreamDestroy(st) == hipSuccess,
                "hipStreamDestroy failed");
  });
  m.def("stream_priority_range", [] {
    int lo = 0, hi = 0;
    hipDeviceGetStreamPriorityRange(&lo, &hi);
    return std::vector<int>{lo, hi};
  });
  m.def("maxpool2d_fwd", &maxpool2d_fwd);
  m.def("maxpool2d_bwd", &maxpool2d_bwd);
  m.def("avgpool_fwd", &avgpool_fwd);
  m.def("avgpool_bwd", &avgpool_bwd);

  // -------------------------------------------------------------- RCCL
  py::class_<RcclWork, std::shared_ptr<RcclWork>>(m, "RcclWork")
      .def("wait", &RcclWork::wait)
      .def("synchronize", &RcclWork::synchronize, py::call_guard<py::gil_scoped_release>())
      .def("is_completed", &RcclWork::is_completed);

  py::class_<RcclComm, std::shared_ptr<RcclComm>>(m, "RcclComm")
      .def_static("unique_id", [] { return py::bytes(RcclComm::unique_id()); })
      .def(py::init([](py::bytes uid, int rank, int world, int device, double timeout) {
             std::string id = uid;  // copy while holding the GIL
             py::gil_scoped_release nogil;
             return std::make_shared<RcclComm>(id, rank, world, device, timeout);
           }),
           py::arg("uid"), py::arg("rank"), py::arg("world"), py::arg("device"), py::arg("timeout") = 1800.0)
      .def_property_readonly("rank", &RcclComm::rank)
      .def_property_readonly("size", &RcclComm::size)
      .def_property_readonly("device", &RcclComm::device)
      .def_property_readonly("stream_ptr", [](RcclComm& c) { return reinterpret_cast<intptr_t>(c.stream()); })
      .def_property_readonly("stream_kind", &RcclComm::stream_kind)
      .def("count", &RcclComm::count)
      .def("healthy", &RcclComm::healthy)
      .def("error", &RcclComm::error)
      .def("abort", &RcclComm::abort)
      .def("shutdown", &RcclComm::shutdown, py::call_guard<py::gil_scoped_release>())
      .def("set_timeout", &RcclComm::set_timeout)
      .def("set_test_postop", &RcclComm::set_test_postop, py::arg("delay_us"), py::arg("scale"),
           "test hook: delay + scale after every all_reduce, inside its completion event")
      .def("set_test_postop_model", &RcclComm::set_test_postop_model, py::arg("alpha_us"), py::arg("gbps"),
           py::arg("world"), "test hook: modelled ring all-reduce time after every all_reduce (one-GPU stand-in)")
      .def("timeout", &RcclComm::timeout)
      .def("captured_collectives", &RcclComm::captured_collectives)
      .def("eager_collectives", &RcclComm::eager_collectives)
      .def("all_reduce", &RcclComm::all_reduce, py::arg("t"), py::arg("op") = "sum", py::arg("async_op") = false)
      .def("broadcast", &RcclComm::broadcast, py::arg("t"), py::arg("root") = 0, py::arg("async_op") = false)
      .def("reduce", &RcclComm::reduce, py::arg("t"), py::arg("root") = 0, py::arg("op") = "sum",
           py::arg("async_op") = false)
      .def("all_gather", &RcclComm::all_gather, py::arg("out"), py::arg("inp"), py::arg("async_op") = false)
      .def("reduce_scatter", &RcclComm::reduce_scatter, py::arg("out"), py::arg("inp"), py::arg("op") = "sum",
           py::arg("async_op") = false)
      .def("gather", &RcclComm::gather, py::arg("t"), py::arg("outs"), py::arg("root") = 0,
           py::arg("async_op") = false)
      .def("scatter", &RcclComm::scatter, py::arg("t"), py::arg("ins"), py::arg("root") = 0,
           py::arg("async_op") = false)
      .def("all_to_all", &RcclComm::all_to_all, py::arg("out"), py::arg("inp"), py::arg("async_op") = false)
      .def("send", &RcclComm::send, py::arg("t"), py::arg("peer"), py::arg("async_op") = false)
      .def("recv", &RcclComm::recv, py::arg("t"), py::arg("peer"), py::arg("async_op") = false)
      .def("barrier", &RcclComm::barrier, py::call_guard<py::gil_scoped_release>());

  // -------------------------------------------------------------- reducer
  py::class_<Reducer, std::shared_ptr<Reducer>>(m, "Reducer")
      .def(py::init<std::vector<at::Tensor>, std::vector<at::Tensor>, std::vector<at::Tensor>, std::vector<int64_t>,
                    std::shared_ptr<RcclComm>, c10::intrusive_ptr<c10d::ProcessGroup>, bool, bool>(),
           py::arg("params"), py::arg("grad_views"), py::arg("bucket_views"), py::arg("bucket_starts"),
           py::arg("rccl"), py::arg("pg"), py::arg("find_unused"), py::arg("average"))
      .def("prepare_for_backward", &Reducer::prepare_for_backward)
      .def("remove_hooks", &Reducer::remove_hooks)
      .def("ready_order", &Reducer::ready_order)
      .def("disarm", &Reducer::disarm)
      .def("set_defer", &Reducer::set_defer)
      .def("set_trace", &Reducer::set_trace)
      .def("trace_log", &Reducer::trace_log)
      .def_property_readonly("iterations", &Reducer::iterations)
      .def_property_readonly("launched_total", &Reducer::launched_total)
      .def_property_readonly("num_buckets", &Reducer::num_buckets)
      .def("set_bucket_step", &Reducer::set_bucket_step, py::arg("bucket"), py::arg("p"), py::arg("g"), py::arg("buf"),
           py::arg("lr_t"), py::arg("lr"), py::arg("momentum"), py::arg("dampening"), py::arg("wd"), py::arg("nesterov"),
           py::arg("first"), py::arg("maximize"), py::arg("desc") = py::none(), py::arg("meta") = py::none(),
           py::arg("amax") = py::none(), py::arg("counter") = py::none(),
           "SGD over bucket b's arena range, run on the reducer's step stream as soon as b's all-reduce completes "
           "(held for the next backward only)")
      .def("clear_bucket_steps", &Reducer::clear_bucket_steps)
      .def("set_post_broadcast", &Reducer::set_post_broadcast, py::arg("tensors"))
      .def("join_post_broadcast", &Reducer::join_post_broadcast)
      .def("take_post_issued", &Reducer::take_post_issued)
      .def_property_readonly("stepped_buckets", &Reducer::stepped_buckets);
}
