/* libdepgan -- C ABI of the MI355X-native DEP-GAN two-critic WGAN-GP hot path.
 *
 * The reference (febrianrachmadi/dep-gan-im) has no FFI: its boundary is the
 * slice of the Keras API that DEP-GAN_PROB_IM_twoCritics_training_4fold.py
 * ("GT") touches.  Each entry point below names the reference construct it
 * replaces.  All pointers are plain device (HIP) or host pointers, no
 * framework types.  Every function returns 0 on success; on failure
 * depgan_last_error() describes what went wrong.  A context is not thread safe;
 * independent contexts (one per rank / GPU) are.
 *
 * Tensors are NHWC fp32, Keras weight layouts (Conv2D HWIO, Conv2DTranspose
 * (kh,kw,Cout,Cin), Dense (in,out)).
 */
#ifndef DEPGAN_H
#define DEPGAN_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct depgan_ctx depgan_ctx;

/* ABI guard: bump when depgan_config or the meaning of an entry point changes.  depgan_create rejects a
 * depgan_config whose struct_size is not sizeof(depgan_config) of THIS header (a caller compiled or bound against an
 * older layout would otherwise make the library read past its struct). */
#define DEPGAN_ABI_VERSION 3
int depgan_abi_version(void);
size_t depgan_config_size(void);
/* first 32 hex digits of the sha256 over the sources this binary was built from (dep_gan_im_amd/build.py::source_hash):
 * the Python binding compares it with the sources lying next to it and refuses a stale library */
const char* depgan_source_hash(void);

typedef struct depgan_config {
  int struct_size;  /* = sizeof(depgan_config); checked by depgan_create                */
  int batch;        /* per-device batch size (batchSize, GT:42)                       */
  int height;       /* imageSize (GT:40); must be a multiple of 16                    */
  int width;
  int nicg;         /* generator input channels (GT:22)                               */
  int first_fm;     /* first_fm_G (GT:35); 32                                          */
  float im_thresh;  /* IM_TRSH (GT:25-29)                                              */
  float delta;      /* WGAN-GP weight (GT:37)                                          */
  float lrD, lrG;   /* GT:44-45                                                        */
  float beta1, beta2, adam_eps; /* Adam(beta_1=0, beta_2=0.9), K.epsilon() (GT:549)    */
  int nc_out;       /* generator head channels: 1 = DEP-GAN (tanh, GT:520); 2..DEPGAN_MAX_HEAD_CLASSES = DEP-UResNet
                       with that many classes (softmax; the reference's n_label = 4, UT:573, 583).  0 is read as 1;
                       anything else is refused.  The bound of 8 lets a pixel's logits, probabilities and gradient
                       live in registers as two float4.                                   */
  int bf16_weights; /* BASELINE config 4: 1 = every "/kernel" tensor is rounded to bf16 (RNE) before use, products
                       accumulate in fp32, the fp32 master copy and the Adam state stay fp32; 0 = fp32 weights */
  int bf16_mfma;    /* BASELINE config 4 on the bf16 matrix pipe (needs bf16_weights = 1): the MFMA convolutions AND the
                       weight-gradient contractions round their operands to bf16 (RNE) while staging them and run
                       v_mfma_f32_32x32x16_bf16 with fp32 accumulation; everything between them stays fp32.
                       0 = fp32 matrix pipe.
                       With nc_out >= 2 it creates an INFERENCE CONTEXT: the DEP-UResNet in learning phase 0 only
                       (depgan_g_forward, depgan_g_forward_bf16s, the weight entry points).  It holds no critics,
                       gradient tensors, phase-1 buffers or weight-gradient slab, and every training entry
                       (depgan_uresnet_*, depgan_apply_adam, the WGAN-GP closures, depgan_d_forward and the
                       depgan_set_*_storage / _pipe setters) returns status 3 before any launch  */
  int f32_split;    /* 0 (default): fp32 products on v_mfma_f32_32x32x2_f32.  6 or 3 (opt-in, never the benchmark's
                       headline; excludes bf16_weights / bf16_mfma): every fp32 operand of the MFMA convolutions is split
                       exactly into three (two) bf16 terms and the six (three) largest cross products run on
                       v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- dropped terms are below 2^-24 (2^-16) of
                       |x||w|, i.e. fp32-grade (6) or TF32-grade-plus (3) products at 2.7x (5.3x) the fp32 matrix rate */
} depgan_config;
#define DEPGAN_MAX_HEAD_CLASSES 8

enum { DEPGAN_NET_G = 0, DEPGAN_NET_D_Y2 = 1, DEPGAN_NET_D_DEM = 2 };
enum { DEPGAN_ARENA_PARAMS = 0, DEPGAN_ARENA_NONTRAINABLE = 1, DEPGAN_ARENA_GRADS = 2,
       DEPGAN_ARENA_ADAM_M = 3, DEPGAN_ARENA_ADAM_V = 4 };

const char* depgan_last_error(void);

/* Gen_UNet2D(...) + 2 x Dis_C2D_FCN1(...) + the loss graph of GT:513-598.
 * Weights start zeroed: load them with depgan_arena_ptr + depgan_weights_changed. */
int depgan_create(const depgan_config* cfg, depgan_ctx** out);
void depgan_destroy(depgan_ctx* ctx);
/* all work is enqueued on this hipStream_t (default: the null stream).  The stream contract ("Streams"):
 *   - Every kernel, memset and copy of a context entry goes to the stream set here; every stateless entry that takes a
 *     `stream` / `hip_stream` argument puts all its work on that stream.  Nothing is enqueued on the null stream and no
 *     entry waits for it, so a stream created non-blocking (hipStreamNonBlocking, torch.cuda.Stream()) is supported:
 *     operands need only be valid in that stream's order, not on the host's clock.
 *   - An entry that returns host values (losses, counts, a status that depends on device data) synchronises that stream
 *     and no other; an entry that returns none does not wait for the device at all.
 *   - Allocation is the one exception and it is closed on return: depgan_create and every entry that allocates context
 *     memory lazily (depgan_set_fwd_only_storage / depgan_set_g_update_storage and the first pass under them,
 *     depgan_g_forward_bf16s, depgan_set_optimizer, the first capture under depgan_debug_capture) zero-fill on the null
 *     stream and wait for it once before they return.
 *     On return every zero-fill and table upload is complete on the device, whatever stream the next kernel -- or the
 *     caller's own upload through depgan_arena_ptr -- runs on.
 *   - depgan_set_stream itself enqueues nothing and waits for nothing.  Ordering across a switch is the caller's job:
 *     work already enqueued on the old stream must be finished (or the new stream made to wait for it) before an entry
 *     on the new stream touches the context. */
int depgan_set_stream(depgan_ctx* ctx, void* hip_stream);

/* Data parallelism (the reference is single-GPU, GT:13).  The library stays free of any communication
 * dependency: the host registers ONE function that all-reduces (sum) n device floats in place across the ranks,
 * ENQUEUED on hip_stream (RCCL via torch.distributed in dep_gan_im_amd/dist.py); it must not synchronise the host.
 * With a hook registered every *_step / depgan_gen_iteration / depgan_g_eval_multi call all-reduces, per network
 * update, that network's gradient arena together with the un-normalised loss pieces (one message), divides the
 * gradient by `world` inside Adam and reports GLOBAL scalars, identical on every rank (hence the same best-of-k
 * noise choice).  *_grads calls never communicate.  fn == NULL removes the hook; world = 1 with a hook is a one-rank
 * job (the hook is still called). */
typedef int (*depgan_allreduce_fn)(void* user, float* dev_ptr, long n, void* hip_stream);
int depgan_set_allreduce(depgan_ctx* ctx, depgan_allreduce_fn fn, void* user, int world);

/* Direct RCCL binding ("ncclAllReduce ... one call per network per step").  The library calls
 * ncclAllReduce(arena, nTrain + 8, ncclFloat, ncclSum, comm, stream) itself, on the context's stream, for every network
 * update (and once per best-of-k evaluation block); librccl is resolved at run time -- the copy already loaded in the
 * process (PyTorch-ROCm ships one), else dlopen("librccl.so.1") -- so libdepgan.so has no link dependency on it.
 *   depgan_rccl_unique_id:  rank 0 creates the 128-byte ncclUniqueId; the host hands it to every rank by any means
 *                           (dep_gan_im_amd/dist.py: one torch.distributed broadcast of the bytes).
 *   depgan_rccl_init:       collective over all ranks: ncclCommInitRank on the context's device.  Replaces a hook
 *                           registered with depgan_set_allreduce; from then on the closures behave as described there
 *                           (global scalars, gradients divided by `world` inside Adam).  world = 1 is a one-rank job.
 *   depgan_rccl_broadcast:  ncclBroadcast of n device floats from `root`, enqueued on the context's stream (replica
 *                           initialisation: rank 0's weights, BN statistics and Adam state).
 *   depgan_rccl_info:       communicator size and rank as RCCL reports them (ncclCommCount / ncclCommUserRank) and
 *                           the number of collectives this context has issued.
 *   depgan_rccl_shutdown:   ncclCommDestroy (depgan_destroy does it as well). */
#define DEPGAN_RCCL_ID_BYTES 128
int depgan_rccl_unique_id(void* id_out);
int depgan_rccl_init(depgan_ctx* ctx, const void* id, int rank, int world);
int depgan_rccl_broadcast(depgan_ctx* ctx, float* dev_ptr, long n, int root);
int depgan_rccl_info(depgan_ctx* ctx, int* nranks, int* rank, long* collectives_issued);
int depgan_rccl_shutdown(depgan_ctx* ctx);

/* model.trainable_weights / get_weights / set_weights (GT:549, 892; GE:383) */
int depgan_param_count(depgan_ctx* ctx, int net);
int depgan_param_info(depgan_ctx* ctx, int net, int index, char* name, int name_cap, int shape[4], int* ndim,
                      long* offset, int* trainable);
long depgan_arena_floats(depgan_ctx* ctx, int net, int arena);
float* depgan_arena_ptr(depgan_ctx* ctx, int net, int arena); /* device pointer */
/* call after writing into a PARAMS / NONTRAINABLE arena from outside */
int depgan_weights_changed(depgan_ctx* ctx, int net);

/* Model.predict (GT:846-848, 859; GE:621): n <= batch samples, learning phase 0 */
int depgan_g_forward(depgan_ctx* ctx, const float* x_dev, const float* z_dev, float* out_dev, int n);
int depgan_d_forward(depgan_ctx* ctx, int net, const float* img_dev, float* out_dev, int n);

/* netD_y2_train / netD_dem_train ([y2, x, z, ep] -> [loss_real, loss_fake]; GT:550-552, 569-571).
 * *_grads leaves d loss / d theta_D in the GRADS arena without updating (so a
 * data-parallel caller can all-reduce it), depgan_apply_adam applies
 * Adam.get_updates (GT:549, 568, 594); *_step does both. */
int depgan_critic_grads(depgan_ctx* ctx, int net, const float* y2_dev, const float* x_dev, const float* z_dev,
                        const float* ep_dev, float out_host[2]);
int depgan_critic_step(depgan_ctx* ctx, int net, const float* y2_dev, const float* x_dev, const float* z_dev,
                       const float* ep_dev, float out_host[2]);
/* netG_no_update / netG_train ([x, y2, z] -> [loss, loss_fake, loss_fake_dem, M1, M3, M4]; GT:595-598) */
int depgan_g_eval(depgan_ctx* ctx, const float* x_dev, const float* y2_dev, const float* z_dev, float out_host[6]);
int depgan_g_grads(depgan_ctx* ctx, const float* x_dev, const float* y2_dev, const float* z_dev, float out_host[6]);
/* The best-of-k noise search of the driver (GT:868-877: k = 10 calls of netG_no_update on the SAME batch with k
 * noises, then argmin of the total loss): k evaluations enqueued back to back, one host synchronisation.
 * z_all_dev: (k, batch, 32) ; out_host: k x 6 scalars as depgan_g_eval ; sums_host (may be NULL): k x 8
 * un-normalised pieces as depgan_last_sums (for the data-parallel combine).  1 <= k <= DEPGAN_MAX_MULTI. */
#define DEPGAN_MAX_MULTI 32
int depgan_g_eval_multi(depgan_ctx* ctx, const float* x_dev, const float* y2_dev, const float* z_all_dev, int k,
                        float* out_host, float* sums_host);
int depgan_g_step(depgan_ctx* ctx, const float* x_dev, const float* y2_dev, const float* z_dev, float out_host[6]);
int depgan_apply_adam(depgan_ctx* ctx, int net);
/* Adam `iterations` of a network's optimiser (GT:549, 568, 594), for checkpoint / resume */
long depgan_get_adam_step(depgan_ctx* ctx, int net);
int depgan_set_adam_step(depgan_ctx* ctx, int net, long t);

/* Optimiser options of one network (DEPGAN_NET_*), off by default.  With none set every update launches the plain Adam
 * kernel with the arguments it always had.
 * depgan_set_lr / depgan_get_lr: the learning rate the network was created with (lrG / lrD), settable at any time; it
 *   takes effect at the next update.  Host only.  lr finite and > 0, else status 1.
 * depgan_set_optimizer(ctx, net, clipnorm, clipvalue, weight_decay): each finite and >= 0, 0 = off; a negative, NaN or
 *   infinite value is status 1 before any HIP call, an inference context status 3.  All three 0 is the plain path again.
 *   Every update of the network (depgan_apply_adam, depgan_uresnet_step*, the critic and generator steps,
 *   depgan_gen_iteration) then runs, on the gradient g' = g * gscale the plain update uses (gscale = 1 / world after a
 *   summing all-reduce, so the globally averaged gradient):
 *     clipnorm = c:     norm = sqrt(sum_i (double)g'_i^2), a deterministic two-stage reduction enqueued in front of the
 *                       update; s = norm >= c ? (float)(c / norm) : 1; g'' = g' * s (standalone Keras 2's clipnorm: one
 *                       global norm).  The update kernel reads the norm on the device, no host synchronisation is
 *                       added.  If the squared norm is not finite (a NaN or an infinity in the gradient) the update
 *                       writes nothing: parameters and both Adam moments keep their bits.  The step counter
 *                       (depgan_get_adam_step) has advanced all the same.
 *     clipvalue = a:    g'' = min(max(g'', -a), a), after the norm scaling.
 *     weight_decay = w: decoupled decay (AdamW): p <- p - (lr * w) p before the Adam displacement, with the plain lr
 *                       (not the bias-corrected one), on the tensors whose name ends in "/kernel" (convolution,
 *                       transposed-convolution and dense kernels); biases and BatchNorm gamma / beta are never decayed.
 *   depgan_get_optimizer returns 1 and the three values with an option on, 0 (and zeros) otherwise.
 * depgan_last_grad_norm: norm and s of the network's last update made with clipnorm on (s = 0: the update was refused,
 *   norm is then not finite).  Synchronises the stream.  Status 1 before any such update. */
int depgan_set_lr(depgan_ctx* ctx, int net, float lr);
int depgan_get_lr(depgan_ctx* ctx, int net, float* lr);
int depgan_set_optimizer(depgan_ctx* ctx, int net, float clipnorm, float clipvalue, float weight_decay);
int depgan_get_optimizer(depgan_ctx* ctx, int net, float* clipnorm, float* clipvalue, float* weight_decay);
int depgan_last_grad_norm(depgan_ctx* ctx, int net, double* norm, float* scale);

/* One generator iteration of the reference schedule (GT:791-829, 868-878) with ONE host synchronisation:
 *   n_y2  critic-Y2 updates  on the batches  x_y2 + j*stride, y2_y2 + j*stride_y   (j = 0 .. n_y2-1)   GT:802-814
 *   n_dem critic-DEM updates on the batches  x_dem + j*stride, ...                                        GT:817-829
 *   k evaluations of the generator loss on (x_gen, y2_gen) with the noises z_gen[0..k)                    GT:868-874
 *   arg-min of the total loss (first minimum of the float32 values, as np.argmin)                         GT:875-876
 *   one generator update with that noise                                                                  GT:878
 * everything enqueued back to back (the arg-min and the noise gather run on the device), all scalars fetched at the
 * end.  batch_stride = samples between the starts of consecutive batches (batch for data resident in HBM as one
 * array; world*batch when the rank takes every world-th batch).  z_*: (n, batch, 32), ep_*: (n, batch).
 * out_host: n_y2 x 2 [loss_real, loss_fake], then n_dem x 2, then k x 6, then the 6 scalars of the update
 * (2 n_y2 + 2 n_dem + 6 k + 6 floats); *best_host = chosen noise index.  n_y2, n_dem >= 0, 1 <= k <= DEPGAN_MAX_MULTI;
 * n_y2 + n_dem <= DEPGAN_MAX_CRITIC_STEPS. */
#define DEPGAN_MAX_CRITIC_STEPS 256
int depgan_gen_iteration(depgan_ctx* ctx, const float* x_y2, const float* y2_y2, const float* z_y2, const float* ep_y2,
                         int n_y2, const float* x_dem, const float* y2_dem, const float* z_dem, const float* ep_dem,
                         int n_dem, long batch_stride, const float* x_gen, const float* y2_gen, const float* z_gen, int k,
                         float* out_host, int* best_host);

/* DEP-UResNet supervised path (DEP-UResNet-wNoises-training-4fold.py "UT"; contexts created with nc_out = C in
 * 2..DEPGAN_MAX_HEAD_CLASSES and bf16_mfma = 0):
 * my_network.fit / train_on_batch (UT:427, 602-606) = learning phase 1: batch-statistics BatchNorm with
 * moving-average updates, Dropout(0.25) after conv_10 (UT:388; drop_seed 0 disables it), softmax +
 * categorical cross-entropy, Adam(beta1, beta2 of the config).  labels: one-hot (n,H,W,C) fp32.
 * n: samples in this call (1..batch; the last batch of a keras epoch may be short); loss_host: mean loss.
 * depgan_uresnet_grads leaves the gradients in the G arena and, like any phase-1 forward pass, moves
 * the BN moving statistics; depgan_uresnet_step also applies Adam.                                   */
int depgan_uresnet_grads(depgan_ctx* ctx, const float* x_dev, const float* z_dev, const float* labels_dev, int n,
                         unsigned drop_seed, float* loss_host);
int depgan_uresnet_step(depgan_ctx* ctx, const float* x_dev, const float* z_dev, const float* labels_dev, int n,
                        unsigned drop_seed, float* loss_host);
/* validation loss in learning phase 0 (UT:606); n in 1..batch */
int depgan_uresnet_eval(depgan_ctx* ctx, const float* x_dev, const float* z_dev, const float* labels_dev, int n,
                        float* loss_host);
/* The same three entries with integer labels (keras sparse_categorical_crossentropy): codes_dev is (n,H,W) unsigned
 * char, one class index per pixel, 1 byte where the one-hot tensor has 4 C.  The cross-entropy kernel forms the one-hot
 * row in registers and runs the one-hot statements, so every result equals, bit for bit, that of the one-hot entry fed
 * the one-hot encoding of the codes.  A code is only compared, never used as an index: any byte value is safe.  Pixels
 * whose code is outside [0, C) add neither loss nor gradient and are counted on the device; the count comes back with
 * the loss (the one synchronisation these entries have), and if it is not zero the entry returns status 1 with a
 * message that gives it.  depgan_uresnet_step_sparse then applies NO Adam update and leaves the Adam step counter
 * alone; the phase-1 forward has by then moved the BatchNorm moving statistics, as depgan_uresnet_grads always does. */
int depgan_uresnet_grads_sparse(depgan_ctx* ctx, const float* x_dev, const float* z_dev, const unsigned char* codes_dev,
                                int n, unsigned drop_seed, float* loss_host);
int depgan_uresnet_step_sparse(depgan_ctx* ctx, const float* x_dev, const float* z_dev, const unsigned char* codes_dev,
                               int n, unsigned drop_seed, float* loss_host);
int depgan_uresnet_eval_sparse(depgan_ctx* ctx, const float* x_dev, const float* z_dev, const unsigned char* codes_dev,
                               int n, float* loss_host);

/* The class census of the supervised path: accuracy, Dice and IoU of a batch from the pass that computes its loss.
 * depgan_uresnet_set_census(ctx, 1): from now on every depgan_uresnet_{grads,step,eval}{,_sparse} call also counts, in
 *   the softmax + cross-entropy kernel itself, the pixels of every (true class, predicted class) pair -- the definitions
 *   of depgan_op_softmax_ce_census: predicted = first arg-max of the probabilities (a tie goes to the lower index),
 *   true = the code, or the first arg-max of the one-hot row.  Default 0.  The loss, the gradients and every other result
 *   are bit for bit what they are with the census off.  on = 1 is refused before any launch on a context without the
 *   trainable softmax head: status 3 on an inference context, status 1 for nc_out = 1; a value other than 0 or 1 is
 *   status 1.  depgan_uresnet_get_census returns the setting.
 * depgan_uresnet_last_census: host only.  out_host[tc * C + pc] (C = nc_out, reported in *classes when not NULL; the
 *   first C*C entries are valid) = the table of the last depgan_uresnet_* call made with the census on.  It came back in
 *   the same copy and synchronisation as that call's loss.  Status 1 before any such call and after set_census(0).
 *   What a call counts: grads / step count the phase-1 predictions the loss is taken from -- batch-statistics BatchNorm
 *   and Dropout included, made BEFORE the Adam update -- which is what Keras' training metrics see; eval counts the
 *   phase-0 predictions, the arg-max of depgan_g_forward on the same inputs.  A pixel whose code is outside [0, C) is in
 *   no bin: the table sums to n*H*W minus the count the refused call reports, and a sparse step refused for such codes
 *   still leaves its table here. */
int depgan_uresnet_set_census(depgan_ctx* ctx, int on);
int depgan_uresnet_get_census(depgan_ctx* ctx);
int depgan_uresnet_last_census(depgan_ctx* ctx, long long out_host[DEPGAN_MAX_HEAD_CLASSES * DEPGAN_MAX_HEAD_CLASSES],
                               int* classes);

/* The loss-weight mode of the supervised path: per-class loss weights and a label that takes a pixel out of the loss.
 * depgan_uresnet_set_loss_weights(ctx, w_host, n, ignore_code): w_host = nc_out class weights cw[k] on the host, each
 *   finite and >= 0, at least one > 0, n == nc_out; ignore_code = -1 for none, else a byte value 0..255 (it may be
 *   >= nc_out, or a real class).  Anything else is status 1 with a message, before any HIP call; status 3 on an inference
 *   context, status 1 for nc_out = 1 (as depgan_uresnet_set_census).  w_host == NULL turns the mode off (the default):
 *   every entry then computes, bit for bit, what it computed before this mode existed.
 * With the mode on, all six depgan_uresnet_{grads,step,eval}{,_sparse} entries use, per pixel with label row t (the
 *   one-hot row, or t[k] = (k == code) formed in registers):
 *     a code equal to ignore_code has t = 0 and is NOT counted as out of range; any other code >= nc_out is counted and
 *     refused as before; with one-hot labels the ignored pixel is the all-zero row (the ignore code is not read);
 *     pixel weight w_i = sum_k cw[k] t[k] (left to right); den = the number of pixels with w_i != 0, an exact integer
 *     counted by a label pre-pass on the device; loss = -sum_i sum_k cw[k] t[k] log r_k / den, q and r as in
 *     depgan_op_softmax_ce; dL/dq_k = -cw[k] t[k] (1/den) / q_k on the closed clip interval.
 *   This is Keras 2's weighted-objective rule (the weighted sum over the count of non-zero weights), not a division by
 *   sum w_i.  Ignored pixels and pixels of a zero-weight class add no loss and no gradient (their dz row is 0), are not
 *   in den, and still get their probabilities.  den == 0: loss 0.0, dz all zero, status 0; depgan_uresnet_step{,_sparse}
 *   then applies NO Adam update and leaves the step counter alone (the moving statistics have moved).  *loss_host =
 *   sum / den and depgan_last_sums[1] = den.  Census: a pixel without a true class (the ignore code, an all-zero one-hot
 *   row) joins no bin, a zero-weight class keeps its bin: sum(table) + out-of-range + ignored == n*H*W.
 * depgan_uresnet_get_loss_weights: returns 1 and fills w_host (nc_out entries) and *ignore_code (either may be NULL)
 *   when the mode is on, else returns 0.
 * depgan_uresnet_last_label_counts: host only.  out_host = the pre-pass counts of the last depgan_uresnet_* call made
 *   with the mode (or the focal mode, depgan_uresnet_set_focal) on, which came back in the same copy and synchronisation as its loss: [0] den, [1] pixels without a
 *   true class, [2] out-of-range codes, [3 + k] pixels of true class k (the code, or the first arg-max of the one-hot
 *   row); the first nc_out + 3 entries are valid, nc_out reported in *classes when not NULL.  Status 1 before any such
 *   call and after the mode was set again. */
#define DEPGAN_LABEL_NCOUNT 11 /* 3 + DEPGAN_MAX_HEAD_CLASSES */
int depgan_uresnet_set_loss_weights(depgan_ctx* ctx, const float* w_host, int n, int ignore_code);
int depgan_uresnet_get_loss_weights(depgan_ctx* ctx, float w_host[DEPGAN_MAX_HEAD_CLASSES], int* ignore_code);
int depgan_uresnet_last_label_counts(depgan_ctx* ctx, long long out_host[DEPGAN_LABEL_NCOUNT], int* classes);

/* The soft Dice loss of the supervised path, alone or added to the cross-entropy (the reference's dice_coef_loss,
 * UT:110-121, and a per-class form).  With p the softmax probabilities AS STORED (not the renormalised, clipped q of the
 * cross-entropy), t the label row (the one-hot row, or t[k] = (k == code) formed in registers), m = 1 for a pixel that
 * takes part and 0 otherwise, s = smooth, over the pixels of the call:
 *     I_k = sum_i m t_k p_k      P_k = sum_i m p_k      T_k = sum_i m t_k
 *   DEPGAN_DICE_FLAT:   L = 1 - (2 sum_k I_k + s) / (sum_k T_k + sum_k P_k + s)
 *   DEPGAN_DICE_CLASS:  L = sum_k c_k (1 - D_k),  D_k = (2 I_k + s) / (T_k + P_k + s),  class coefficients c_k >= 0
 *     (c_k = 1/C: one minus the mean class Dice; c_0 = 0, c_k = 1/(C-1): the foreground Dice).
 *   The loss of a call is ce_coef * CE + dice_coef * L, CE = what the context computes without this mode (the plain mean,
 *   or the loss-weight mode's sum / den); the gradient is the same combination.
 * Which pixels take part: with the loss-weight mode off, every pixel.  With it on, a pixel without a true class (the
 *   ignore code, an all-zero one-hot row) has m = 0: it is in none of the sums and gets no Dice gradient.  A code >= nc_out
 *   that is not the ignore code has m = 0 too; it is counted and the call refused as without this mode.  The class weights
 *   of the loss-weight mode act on the cross-entropy alone.  No pixel takes part: L = 0.0 with a zero gradient, and
 *   depgan_uresnet_step{,_sparse} applies NO Adam update and leaves the step counter alone (then the cross-entropy has
 *   den == 0 as well).  A batch with den == 0 whose pixels of zero-weight classes take part in L is updated as usual.
 * depgan_uresnet_set_dice_loss(ctx, form, ce_coef, dice_coef, smooth, class_coef_host, n): form = DEPGAN_DICE_OFF (the
 *   default; the other arguments are not read) restores, bit for bit, what every entry computed before this mode existed.
 *   Otherwise ce_coef finite and >= 0, dice_coef finite and > 0, smooth finite and > 0 (so no denominator is 0);
 *   class_coef_host = NULL (1/nc_out each), or n == nc_out host values, finite and >= 0 with at least one > 0; it must
 *   be NULL for the flat form.  Anything else is status 1 with a message, before any HIP call; status 3 on an inference
 *   context, status 1 for nc_out = 1 (as depgan_uresnet_set_census).
 * With the mode on all six depgan_uresnet_{grads,step,eval}{,_sparse} entries run, behind the cross-entropy kernel on the
 *   same stream: a reduction pass over the stored probabilities and the labels (block partials, no atomics), a one-block
 *   stage that adds the partials in index order in double and forms L and the per-class scalars of
 *   dL/dp_k = m (A_k t_k + B_k) -- class form A_k = -2 c_k / Den_k, B_k = c_k Num_k / Den_k^2; flat form the same with the
 *   global Num, Den and c_k = 1 -- and (grads, step) a pass that writes dz = ce_coef dz + dice_coef p_k (g_k - sum_j p_j g_j),
 *   sums over k left to right.  With ce_coef == 0 that pass does not read dz.  *loss_host = ce_coef * CE + dice_coef * L,
 *   formed on the host from the call's one copy; depgan_last_sums[0..1] keep the cross-entropy's sum and denominator.
 *   The census is untouched.
 * depgan_uresnet_get_dice_loss: returns the form (0 with the mode off) and, where the pointers are not NULL, the
 *   coefficients, smooth and the nc_out class coefficients in use (for the flat form they are not written).
 * depgan_uresnet_last_dice_sums: host only.  out_host = I_0..I_{C-1}, P_0..P_{C-1}, T_0..T_{C-1} (the first 3 C entries,
 *   C = nc_out reported in *classes when not NULL) and *dice_loss = L of the last depgan_uresnet_* call made with the
 *   mode on; they came back in the same copy and synchronisation as that call's loss.  Status 1 before any such call
 *   and after the mode was set again. */
#define DEPGAN_DICE_OFF 0
#define DEPGAN_DICE_FLAT 1
#define DEPGAN_DICE_CLASS 2
int depgan_uresnet_set_dice_loss(depgan_ctx* ctx, int form, float ce_coef, float dice_coef, float smooth,
                                 const float* class_coef_host, int n);
int depgan_uresnet_get_dice_loss(depgan_ctx* ctx, float* ce_coef, float* dice_coef, float* smooth,
                                 float class_coef_host[DEPGAN_MAX_HEAD_CLASSES]);
int depgan_uresnet_last_dice_sums(depgan_ctx* ctx, double out_host[3 * DEPGAN_MAX_HEAD_CLASSES], int* classes,
                                  float* dice_loss);

/* The boundary loss of the supervised path (Kervadec et al., "Boundary loss for highly unbalanced segmentation"): the
 * softmax probabilities AS STORED integrated against the signed distance map of the labels, added to whatever the
 * cross-entropy and the Dice mode compute.  Over a call's n label slices (H, W):
 *   True class of a pixel: the census's -- the code, or the first arg-max of the one-hot row.  With the loss-weight mode
 *     on, a pixel of the ignore code or with an all-zero row has no true class: it takes no part (m = 0) and is a member
 *     of no class.  A code >= nc_out has none either; it is counted and the call refused as without this mode.
 *   Distance: for class k and slice s let S be the pixels of slice s whose true class is k.  For x in S, d(x) is the
 *     distance to the nearest pixel of slice s not in S; for x not in S, to the nearest pixel in S.  d2 = d^2 is exactly
 *     what depgan_eval_edt_sq defines on that slice as a (1, H, W) volume with wy = sy^2, wx = sx^2:
 *     fl(fl(dx^2 wx) + fl(dy^2 wy)) minimised over the candidate pixels, in double.  Slices never see each other.
 *   phi_k(x) = float32(sqrt(d2)) outside S and float32(-(sqrt(d2) - inside_offset)) inside, root and subtraction in
 *     double, one rounding to float32; an infinite d2 (the class absent from the slice, or filling it) gives 0.
 *     inside_offset in [0, min(sy, sx)]: 0 is the symmetric map, 1 at unit spacing the map of the published code.
 *   L_B = (1/M) sum_x m(x) sum_k c_k phi_k(x) p_k(x), M = the number of pixels that take part, c_k >= 0.
 *     L_B IS NEGATIVE at a perfect prediction (the mass sits where phi < 0) and positive for mass far outside: it is a
 *     term to add to a regional loss, never a loss with a minimum of 0.
 *   g_k = m c_k phi_k / M, dz_j += boundary_coef p_j (g_j - sum_k p_k g_k), sums over k left to right, added to what
 *     the cross-entropy and the Dice mode left in dz.  The loss of a call is (what the context computes without this
 *     mode) + boundary_coef * L_B.
 *   M == 0: the term is 0.0, dz is untouched and depgan_uresnet_step{,_sparse} applies NO Adam update and leaves the
 *     step counter alone, by the Dice mode's rule for an empty batch (every pixel without a true class).
 * depgan_uresnet_set_boundary_loss(ctx, on, boundary_coef, class_coef_host, n, sy, sx, inside_offset): on = 0 (the
 *   default; the other arguments are not read) restores, bit for bit, what every entry computed before this mode
 *   existed: nothing of it is launched.  on = 1: boundary_coef finite and >= 0; class_coef_host = NULL (1/nc_out each) or
 *   n == nc_out host values, finite and >= 0 with at least one > 0 (a class with c_k = 0 gets no map); sy, sx finite and
 *   > 0; inside_offset in [0, min(sy, sx)]; height and width within depgan_eval_edt_sq's 1..4096.  Anything else is
 *   status 1 with a message before any launch, the setting and every buffer as they were; status 3 on an inference
 *   context, status 1 for nc_out = 1.  The first call with on = 1 allocates phi (batch*H*W*nc_out floats) and the
 *   distance pass's scratch (2 bytes per pixel and class); no later call and no step allocates, so a schedule may set
 *   another boundary_coef before every epoch.
 * With the mode on all six depgan_uresnet_{grads,step,eval}{,_sparse} entries run, behind the cross-entropy and the Dice
 *   launches: a row pass and a column pass over all slices and switched-on classes (two launches whatever n), one pass
 *   that reads p, phi, the labels and dz and writes dz and one double partial per block, and one block that adds the
 *   partials in index order.  No atomics, nothing to zero between calls.  M is read on the device from the label
 *   pre-pass (M = n*H*W with the loss-weight mode off); L_B and M come back in the call's one copy.  eval runs the
 *   distance pass and the sum, not the gradient write.
 * depgan_uresnet_get_boundary_loss: returns 1 and fills what is not NULL when the mode is on, else returns 0.
 * depgan_uresnet_last_boundary_loss: host only; L_B and M of the last depgan_uresnet_* call made with the mode on.
 *   Status 1 before any such call and after the mode was set again. */
int depgan_uresnet_set_boundary_loss(depgan_ctx* ctx, int on, float boundary_coef, const float* class_coef_host, int n,
                                     double sy, double sx, double inside_offset);
int depgan_uresnet_get_boundary_loss(depgan_ctx* ctx, float* boundary_coef,
                                     float class_coef_host[DEPGAN_MAX_HEAD_CLASSES], double* sy, double* sx,
                                     double* inside_offset);
int depgan_uresnet_last_boundary_loss(depgan_ctx* ctx, double* boundary_loss, long long* taking_part);

/* The focal mode of the supervised path: focal cross-entropy (Lin et al.; Keras' CategoricalFocalCrossentropy) and label
 * smoothing (the label_smoothing= of Keras' CategoricalCrossentropy), two per-pixel shapings of the cross-entropy itself,
 * computed in the one softmax + cross-entropy kernel.
 * depgan_uresnet_set_focal(ctx, gamma, label_smoothing): gamma finite and >= 0, label_smoothing (eps below) finite and in
 *   [0, 1); anything else is status 1 with a message, before any HIP call; status 3 on an inference context, status 1 for
 *   nc_out = 1 (as depgan_uresnet_set_census).  gamma == 0 together with label_smoothing == 0 turns the mode off (the
 *   default): every entry then launches exactly the kernels it launched before this mode existed, bit for bit.
 * With the mode on, all six depgan_uresnet_{grads,step,eval}{,_sparse} entries use, per pixel with label row t (the
 *   one-hot row, or t[k] = (k == code) formed in registers; the ignore code and an all-zero row give t = 0), class
 *   weights cw (the loss-weight mode's, all 1 when that mode is off), C = nc_out, and q, r = clip(q, 1e-7, 1 - 1e-7) and
 *   the closed-interval clip gradient as in depgan_op_softmax_ce:
 *     w_i  = sum_k cw[k] t[k]                       (left to right: the pre-pass's pixel weight)
 *     has  = any t[k] != 0                          (on the row before weighting)
 *     ts_k = w_i ((1 - eps) t[k] + (has ? eps / C : 0))
 *     L_i  = -sum_k ts_k (1 - r_k)^gamma log r_k
 *     dL/dq_k = -ts_k (1/den) [ (1 - r_k)^gamma / q_k - gamma (1 - r_k)^(gamma - 1) log r_k ]  on the closed clip
 *               interval, else 0
 *     loss = sum_i L_i / den
 *   Everything behind dL/dq -- q = p / S, the softmax Jacobian, the dz row store -- is the plain kernel's text.  For
 *   one-hot rows and eps = 0, ts_k = cw[k] t[k]; smoothing is defined on rows with a true class only, and a pixel of a
 *   zero-weight class has w_i = 0 and stays out of loss, gradient and den.  1 - r is formed directly in float32 (inside
 *   the clip 1 - r >= 2^-23); the power is 1, 1 - r and (1 - r)(1 - r) for gamma = 0, 1 and 2 and
 *   exp2f(gamma log2f(1 - r)) otherwise, and (1 - r)^(gamma - 1) is the power over 1 - r.
 * The denominator.  den, the label pre-pass and the ignore code are the loss-weight mode's: den = the number of pixels with
 *   w_i != 0.  The focal mode always runs that weighted path; with the loss-weight mode off it does so with unit weights
 *   and no ignore code.  So den == n*H*W whenever every pixel has a label, but -- THE DIFFERENCE from the plain mean over
 *   n*H*W of the mode off -- an all-zero one-hot row is then an ignored pixel, outside den and outside the census;
 *   den == 0 gives loss 0.0, an all-zero dz, status 0, and depgan_uresnet_step{,_sparse} applies NO Adam update and
 *   leaves the step counter alone.  *loss_host = sum / den, depgan_last_sums[0..1] = the sum and den, and
 *   depgan_uresnet_last_label_counts is valid after a call made with this mode or the loss-weight mode on.
 * What the mode leaves alone: the probabilities stored are bit for bit the plain kernel's; the census's true class is the
 *   arg-max of the original label row (or the code), never of the smoothed row; the Dice mode reads the original labels
 *   and the stored probabilities and combines with this cross-entropy through ce_coef, and whether a pixel takes part in
 *   the Dice term follows the loss-weight mode's setting alone.  Still one copy and one synchronisation per call.
 * What is exact and what is bounded: class codes against their one-hot encoding, census on against off, power-of-two
 *   class weights and den = P / 2 scale dz exactly; against a float64 evaluation of the rule the kernel keeps the plain
 *   kernel's bounds (probabilities 1e-6, dz 1e-5 max|dz|, the loss sum 1e-5 relative).
 * depgan_uresnet_get_focal: returns 1 and fills *gamma and *label_smoothing (either may be NULL) when the mode is on,
 *   else returns 0. */
int depgan_uresnet_set_focal(depgan_ctx* ctx, float gamma, float label_smoothing);
int depgan_uresnet_get_focal(depgan_ctx* ctx, float* gamma, float* label_smoothing);

/* Un-normalised pieces of the last critic / generator evaluation, for exact
 * data-parallel reporting: critic: [sum D(real), sum D(fake), sum (norm-1)^2, n];
 * generator: [sum D_y2(fake), sum D_dem(attr), sum |attr-real_dem|, sum wr, sum wf, sum wr*wf, n, n*H*W]. */
int depgan_last_sums(depgan_ctx* ctx, float out_host[8]);

/* per-kernel-class device timing (HIP events on the context stream) */
int depgan_profile_enable(depgan_ctx* ctx, int on);
/* class 0: MFMA conv (fwd / bwd-data / u-forward), 1: MFMA wgrad, 2: everything else */
int depgan_profile_read(depgan_ctx* ctx, int klass, double* total_ms, long* launches, double* flops);
/* sum over the class's recorded launches of the algorithmic HBM bytes (operands once, results once; class 0 only) */
int depgan_profile_read_bytes(depgan_ctx* ctx, int klass, double* bytes);
int depgan_profile_reset(depgan_ctx* ctx);
/* one CSV row per recorded launch: class,label,ms,gflop,mbytes,kernel (algorithmic GFLOP / MB of the launch; kernel =
 * the template instantiation as rocprofv3 names it, for the MFMA convolution class) */
int depgan_profile_dump(depgan_ctx* ctx, const char* path);

/* ---- evaluation step after the path (DEP-GAN_testing_4fold.py "GE":616-807) ----
 * Stateless; device pointers; work is enqueued on `stream`.  Number types follow the reference's NumPy statements:
 * depgan_eval_accumulate: acc += (double)(pred * mask) (mask may be NULL) -- the float64 running sum (np.zeros,
 *   GE:617) of the n_repeat float32 masked predictions (GE:618-624);  depgan_eval_divide: acc /= divisor in float64
 *   (GE:628: output_img_pred_mean / float(n_repeat)).
 * depgan_eval_counts: the integer census behind the volumes and the six Dice figures (GE:637-790):
 *   x (npix, nicg) float32 input maps, pred (npix) FLOAT64 mean predicted DEM; optional (NULL = absent) code_real
 *   (npix, values 0..3), mask1 / wmh1 / mask2 / wmh2 / prob2 (npix).  fake = clip(x0 + pred, -1, 1) and its
 *   comparisons run in float64 against thr; the float32 arrays x and prob2 are compared against (float)thr, as NumPy
 *   does for a float32 array and a Python float.  out_host:
 *   [0] nnz(mask1*wmh1) [1] nnz(mask2*wmh2) [2] #(x >= thr) [3] #(prob2 >= thr) [4] nnz(mask2*[fake > thr]);
 *   change code of the prediction 1 shrink / 2 grow / 3 stay; then triples
 *   (#both, #real, #fake) for code 1, 2, 3 at [5..13], for code > 0 at [14..16], for code in {1,2} at [17..19]. */
#define DEPGAN_EVAL_NCOUNT 20
int depgan_eval_accumulate(const float* pred_dev, const float* mask_dev, double* acc_dev, long n, void* stream);
int depgan_eval_divide(double* acc_dev, long n, double divisor, void* stream);
int depgan_eval_counts(const float* x_dev, int nicg, const double* pred_dev, const float* code_real_dev,
                       const float* mask1_dev, const float* wmh1_dev, const float* mask2_dev, const float* wmh2_dev,
                       const float* prob2_dev, long npix, double thr, long long out_host[DEPGAN_EVAL_NCOUNT],
                       void* stream);

/* ---- data step in front of the path (DEP-GAN_PROB_IM_twoCritics_training_4fold.py "GT": 93-118 load_data /
 * data_prep, 124-146 map_image_to_intensity_range, 667-723 masking / clamping / channel concat) ----
 * One subject: volumes are device fp32 arrays in NIfTI file order (x fastest: element (x,y,z) at x + X*(y + Y*z)),
 * already cast to float32 as data_prep does.  Writes the training slices x_out (Z, X, Y, nicg) and y2_out (Z, X, Y, 1):
 *   prob_1 = p1*icv1 [*(1 - sl1)] clamped at 0;  flair_1 = f1*icv1 [*(1 - sl1)] mapped to [0,1] by the subject's min /
 *   max (percentile 0);  prob_2 = p2*icv2 [*(1 - sl2)] clamped at 0.  sl1 / sl2 may be NULL (no stroke-lesion mask:
 *   GT:691, 699 skip it when the file is missing); f1 may be NULL when nicg = 1.  Bit-identical to the NumPy statements.
 *   scratch: depgan_data_prep_scratch_floats(X, Y, Z) device floats (needed for nicg = 2).  Enqueued on `stream`. */
size_t depgan_data_prep_scratch_floats(int X, int Y, int Z);
int depgan_data_prep_subject(const float* p1_dev, const float* f1_dev, const float* icv1_dev, const float* sl1_dev,
                             const float* p2_dev, const float* icv2_dev, const float* sl2_dev, int X, int Y, int Z,
                             int nicg, float* x_out_dev, float* y2_out_dev, float* scratch_dev, void* stream);

/* ---- DEP-UResNet data step and evaluation (DEP-UResNet-wNoises-training-4fold.py "UT":434-566,
 * DEP-UResNet_testing_4fold.py "UE":496-717) ----
 * Same conventions as above: device pointers, volumes in NIfTI file order, slices out as (Z, X, Y, C), work enqueued
 * on `stream`, int status.
 * depgan_data_prep_zscore (UT:485-512, UE:496-540): brain = f1*icv1 [*(1 - sl1)] (float32 products in that order);
 *   mean and population std (ddof 0) over the WHOLE volume, zeros outside the brain included, each a float64 sum in a
 *   fixed-order two-stage reduction (no float atomics: the bits repeat from run to run), then rounded to float32;
 *   flair_out (Z, X, Y, 1) = nan_to_num((brain - mean32) / std32) in float32 (NaN -> 0, +-inf -> +-FLT_MAX; an all-zero
 *   volume gives zeros).  sl1 may be NULL; stats_out_dev (float[2], may be NULL) receives (mean32, std32);
 *   scratch: depgan_data_zscore_scratch_floats(X, Y, Z) device floats, 8-byte aligned.
 * depgan_data_mask_slices: out (Z, X, Y, 1) = (vol [* m_a]) [* (1 - sl)], m_a / sl may be NULL; bit-identical to the
 *   NumPy statements (UT brain_wsc_1tp; UE brain_wmh_1tp / _2tp, brain_cod_2tp = code2*icv2 without sl, and
 *   icv_and_sl_mask_1tp / _2tp with vol = icv, m_a = NULL).
 * depgan_labels_to_onehot (UT:563-566): onehot_out (npix, C) float32, row i = one_hot(astype(int)(coded[i])) --
 *   truncation toward zero; a value outside [0, C) (NaN included) is status 1 (reported from a device counter; its row
 *   is all zero), not NumPy's negative-index wrap.  Synchronises `stream`.  1 <= C <= DEPGAN_MAX_CLASSES.
 * depgan_eval_accumulate_channels (UE:553-564): acc[i*C+c] += (double)(pred[i*C+c] * mask[i]) (mask may be NULL);
 *   depgan_eval_divide over npix*C then forms the mean.
 * depgan_eval_label_counts (UE:570-697): label = np.argmax over the C float64 channels of pred (npix, C) -- the first
 *   index wins a tie, so pixels the mask zeroed get label 0; labels_out (npix int8, may be NULL) receives it.
 *   code_real / mask1 / wmh1 / mask2 / wmh2 (npix float32) may be NULL (absent).  out_host:
 *   [0] nnz(mask1*wmh1) [1] nnz(mask2*wmh2) [2] #(label > 0) (not masked again, as UE's vol_out);
 *   then triples (#both, #real, #fake), real = code_real compared in float: for == k, k = 1, 2, 3 at [3..11],
 *   for > 0 at [12..14], for in {1,2} at [15..17].  Synchronises `stream`. */
#define DEPGAN_MAX_CLASSES 127
#define DEPGAN_EVAL_LABEL_NCOUNT 18
size_t depgan_data_zscore_scratch_floats(int X, int Y, int Z);
int depgan_data_prep_zscore(const float* f1_dev, const float* icv1_dev, const float* sl1_dev, int X, int Y, int Z,
                            float* flair_out_dev, float* stats_out_dev, float* scratch_dev, void* stream);
int depgan_data_mask_slices(const float* vol_dev, const float* m_a_dev, const float* sl_dev, int X, int Y, int Z,
                            float* out_dev, void* stream);
int depgan_labels_to_onehot(const float* coded_dev, long npix, int C, float* onehot_out_dev, void* stream);

/* ---- training-time augmentation of a resident slice set: the batch gather, an affine warp and an intensity change in
 * one launch (csrc/augment.hip).  Stateless; device pointers; enqueued on `stream`.
 *   x_src (n_src, H, W, nicg) float32, nicg 1..2.  lab_kind 0: no labels (lab_src / lab_out are not read);
 *   1: class codes, uint8 (n_src, H, W);  2: one-hot float32 (n_src, H, W, C), C = 2..DEPGAN_MAX_HEAD_CLASSES.
 *   index_dev[i] (n longs) is the source slice of output sample i; NULL means i (then n_src >= n).  A value outside
 *   [0, n_src) gives a sample made of the fill values alone (x_fill as it is, no gain / offset; the label fill below)
 *   and reads nothing of the sources.
 *   params_dev (n, DEPGAN_AUG_NPARAM) float32, row i = a00 a01 a02 a10 a11 a12 gain offset.  For output pixel (oy, ox):
 *     sy = (a00*oy + a01*ox) + a02          sx = (a10*oy + a11*ox) + a12
 *     y0 = floorf(sy); fy = sy - y0         x0 = floorf(sx); fx = sx - x0
 *     top = v(y0,x0)*(1-fx) + v(y0,x0+1)*fx       bot = v(y0+1,x0)*(1-fx) + v(y0+1,x0+1)*fx
 *     out = gain*(top*(1-fy) + bot*fy) + offset                            per channel
 *     label: row (floorf(sy+0.5f), floorf(sx+0.5f)) of the source labels, copied bit for bit
 *   every operation a single float32 operation in that order (y0+1 and x0+1 are float32 sums too), so a NumPy float32
 *   restatement gives the same bits.  Any coordinate is accepted, +-inf and NaN included: a tap is compared with the
 *   image and clamped into it before it becomes an index.
 *   border 0 (edge): tap indices are clamped into the image.  border 1 (constant): an image tap outside the image is
 *   x_fill (gain and offset then apply as for any pixel); a label outside it is label_fill for codes (0..255), and for
 *   one-hot the row with 1.0 at label_fill (< C), or the all-zero row -- the ignored pixel of
 *   depgan_uresnet_set_loss_weights -- when label_fill < 0.
 *   Writes x_out (n, H, W, nicg) and lab_out (n, H, W) uint8 / (n, H, W, C) float32.  Status 1: n, H, W or n_src < 1,
 *   nicg, lab_kind, border, C or label_fill outside the ranges above, a required pointer NULL, index_dev NULL with
 *   n_src < n, or an output range that overlaps a source range or the other output.  H, W <= 2^24, H*W < 2^31. */
#define DEPGAN_AUG_NPARAM 8
int depgan_data_augment(const float* x_src, int nicg, const void* lab_src, int lab_kind, int C, const long* index_dev,
                        long n_src, const float* params_dev, int n, int H, int W, int border, float x_fill,
                        int label_fill, float* x_out, void* lab_out, void* stream);
/* depgan_data_augment_fields: depgan_data_augment with an elastic deformation and a smooth multiplicative intensity
 * (bias) field per output sample, in the same single launch.  Every argument of depgan_data_augment means what it means
 * there, and:
 *   fields_dev (n, 3, gh, gw) float32, a control grid per output sample i (not per source slice): plane 0 the row
 *   displacement dy in source pixels, plane 1 the column displacement dx, plane 2 the bias b.  gh, gw in
 *   [4, DEPGAN_AUG_MAX_GRID].  Each plane C is evaluated at every output pixel as a uniform cubic B-spline whose
 *   control cells span the image, (gh-3) x (gw-3) of them:
 *     ky = (float)((double)(gh-3) / (double)(H-1))   (0 when H == 1), kx likewise from gw and W   -- host, rounded once
 *     u  = (float)oy * ky;  c = fminf(floorf(u), (float)(gh-4));  t = u - c       (c_x, t_x the same from ox, kx, gw)
 *     t2 = t*t;  t3 = t2*t;  g = 1 - t
 *     B0 = (g*g)*g;  B1 = (3*t3 - 6*t2) + 4;  B2 = ((3*t2 - 3*t3) + 3*t) + 1;  B3 = t3        (six times the weights)
 *     r[j] = ((B0y*C[c_y][j] + B1y*C[c_y+1][j]) + B2y*C[c_y+2][j]) + B3y*C[c_y+3][j]          j = c_x .. c_x+3
 *     f    = (((B0x*r[c_x] + B1x*r[c_x+1]) + B2x*r[c_x+2]) + B3x*r[c_x+3]) * (1.0f/36.0f)
 *   and with f_dy, f_dx, f_b the three planes' values and sy, sx of depgan_data_augment:
 *     sy' = sy + f_dy          sx' = sx + f_dx
 *     the bilinear taps and weights and the nearest label pixel are depgan_data_augment's statements on sy', sx'
 *     out = gain*((top*(1-fy) + bot*fy) * (1 + f_b)) + offset                  per channel; labels do not see b
 *   every operation a single float32 operation in that order, so a NumPy float32 restatement gives the same bits
 *   (tests/elastic_ref.py), whichever way the kernel shares the r[j] among its lanes.  An all-zero grid gives
 *   depgan_data_augment's bits (x + 0, v * 1).  A field value may be anything, +-inf, NaN and 1e30 included: a tap is
 *   compared with the image and clamped into it as a float before it becomes an index, as for any coordinate.
 *   dense_out: NULL, or (n, H, W, 3) float32 that receives f_dy, f_dx, f_b of every output pixel; a sample whose
 *   index is outside [0, n_src) gets zeros there (and the fill values in x_out / lab_out, as above).
 *   Status 1: as depgan_data_augment, fields_dev NULL, gh or gw outside [4, DEPGAN_AUG_MAX_GRID], or an output range
 *   (x_out, lab_out, dense_out) that overlaps a source range (fields_dev among them) or another output. */
#define DEPGAN_AUG_MAX_GRID 32
int depgan_data_augment_fields(const float* x_src, int nicg, const void* lab_src, int lab_kind, int C,
                               const long* index_dev, long n_src, const float* params_dev, const float* fields_dev,
                               int gh, int gw, int n, int H, int W, int border, float x_fill, int label_fill,
                               float* x_out, void* lab_out, float* dense_out, void* stream);
int depgan_eval_accumulate_channels(const float* pred_dev, const float* mask_dev, double* acc_dev, long npix, int C,
                                    void* stream);
int depgan_eval_label_counts(const double* pred_dev, int C, const float* code_real_dev, const float* mask1_dev,
                             const float* wmh1_dev, const float* mask2_dev, const float* wmh2_dev, long npix,
                             signed char* labels_out_dev, long long out_host[DEPGAN_EVAL_LABEL_NCOUNT], void* stream);

/* ---- per-draw statistics of the stochastic predictions and test-time augmentation (csrc/eval_stats.hip) ----
 * What the n_repeat noise draws say beyond their mean.  Stateless; device pointers; enqueued on `stream`; the host does
 * not synchronise; no atomics (a thread owns its pixel's state).  Every float and double operation below is one
 * correctly rounded operation in the stated order, so a NumPy restatement (tests/eval_stats_ref.py) gives the same bits
 * wherever no log is involved.
 * depgan_eval_accumulate_stats: one call per noise draw, in the place of depgan_eval_accumulate[_channels].
 *   pred_dev (n, H, W, C) float32, this draw's prediction, C = 1..DEPGAN_MAX_HEAD_CLASSES; mask_dev (n, H, W) float32
 *   or NULL; params_dev (n, DEPGAN_AUG_NPARAM) float32 or NULL.  State, zeroed by the caller before the first draw,
 *   each pointer optional (NULL = not kept) except sum_dev: sum_dev, sumsq_dev (npix, C) double, ent_sum_dev (npix)
 *   double, votes_dev (npix, C) uint8, count_dev (npix) uint8, npix = n*H*W.  The caller makes at most 255 draws.
 *   For output pixel t = (i, oy, ox) and channel c:
 *     u_c: without params_dev, pred[t, c].  With params_dev (test-time augmentation) row i is an output-to-source map
 *       in depgan_data_augment's convention -- the output is the original frame, the source is the prediction made on
 *       the warped input -- and sy, sx, y0, x0, fy, fx, the four taps and u_c = top*(1-fy) + bot*fy are that entry's
 *       float32 statements applied to the C channels of sample i.  The gain / offset statement is not applied;
 *       elements 6 and 7 of the row are ignored.  A tap is compared with the sample and clamped into it as a float
 *       before it becomes an index, so nothing outside the sample is read, whatever the coordinate.
 *       border 0 (edge): taps are clamped and every draw counts.  border 1 (valid): the draw takes part at this pixel
 *       only if every tap that carries weight lies inside, in0(y0) && in0(x0) && (fy == 0 || in(y0+1)) &&
 *       (fx == 0 || in(x0+1)) -- exact maps (flips, quarter turns, integer shifts) keep their last row and column --
 *       and otherwise NOTHING of the state is touched for this pixel.  Without params_dev border is not used.
 *     v_c = u_c * mask[t] in float32 (v_c = u_c when mask_dev is NULL), as depgan_eval_accumulate_channels
 *     sum[t, c]   = sum[t, c] + (double)v_c                        (that entry's statement and bits)
 *     sumsq[t, c] = sumsq[t, c] + (double)v_c * (double)v_c        (the product is exact; only the add rounds)
 *     ent_sum[t]  = ent_sum[t] + h,  h = ((0 - t_0) - t_1) - ... in channel order,
 *                   t_c = v_c > 0 ? (double)v_c * log((double)v_c) : 0.0   (natural log in double)
 *     votes[t, argmax_c v_c] += 1   -- the first maximum wins and a NaN counts as the maximum, the rule of
 *                   depgan_eval_label_counts; a pixel the mask zeroed votes for class 0
 *     count[t]    += 1
 *   Status 1, nothing launched: n, H, W < 1, C outside 1..DEPGAN_MAX_HEAD_CLASSES, border not 0 / 1, pred_dev or
 *   sum_dev NULL, ent_sum_dev or votes_dev with C < 2, H or W > 2^24 or H*W >= 2^31, or a state range that overlaps
 *   pred, mask, params or another state range.
 * depgan_eval_finish_stats: one call after the last draw, elementwise per pixel, all arithmetic in double, every
 *   operation rounded on its own.  R = n_draws (1..255), or count[t] where count_dev is given; a pixel with R = 0 gets
 *   0.0 in every output.  In place:
 *     mean = sum / R                                          over sum_dev; with count_dev NULL depgan_eval_divide's bits
 *     var  = max(sumsq / R - mean*mean, 0) * (R / (R - ddof)) over sumsq_dev (may be NULL); ddof 0 or 1; 0 where
 *            R - ddof = 0; max(d, 0) = d < 0 ? 0 : d, so a NaN stays one
 *     expected_entropy = ent_sum / R                          over ent_sum_dev (may be NULL)
 *   and into new arrays (npix) double, each may be NULL:
 *     entropy     = the h statement above applied to the mean row
 *     mutual_info = max(entropy - expected_entropy, 0), the BALD term (needs ent_sum_dev); it is non-negative
 *                   mathematically, the clamp only removes rounding
 *   Status 1, nothing launched: sum_dev NULL, npix < 1, C outside 1..DEPGAN_MAX_HEAD_CLASSES, n_draws outside 1..255,
 *   ddof not 0 / 1, ent_sum_dev, entropy_dev or mutual_info_dev with C < 2, mutual_info_dev without ent_sum_dev, or
 *   two ranges that overlap. */
int depgan_eval_accumulate_stats(const float* pred_dev, const float* mask_dev, const float* params_dev, int border,
                                 int n, int H, int W, int C, double* sum_dev, double* sumsq_dev, double* ent_sum_dev,
                                 unsigned char* votes_dev, unsigned char* count_dev, void* stream);
int depgan_eval_finish_stats(double* sum_dev, double* sumsq_dev, double* ent_sum_dev, const unsigned char* count_dev,
                             double* entropy_dev, double* mutual_info_dev, long npix, int C, int n_draws, int ddof,
                             void* stream);

/* ---- surface distances from an exact distance map (csrc/surface_dist.hip; evaluate.surface_distances) ----
 * Stateless; device pointers; enqueued on `stream`; no atomics.  A volume is (D, H, W) bytes with W contiguous -- what
 * (n, H, W) slices are -- and non-zero means set.  1 <= D, H, W <= 4096 and D*H*W < 2^31.
 * depgan_eval_surface_mask: surf[v] = 1 where set[v] != 0 and at least one face neighbour is unset or lies outside the
 *   volume, else 0.  in_plane 0: the 6 neighbours in the volume (a & ~binary_erosion(a, 6-connected, border_value=0));
 *   in_plane 1: the 4 in the slice (slices are several times thicker than pixels; the WMH challenge's convention).
 * depgan_eval_edt_sq: d2[v] (double) = the exact squared Euclidean distance from v to the nearest set voxel, the minimum
 *   over the set voxels of fl(fl(fl(dx^2 wx) + fl(dy^2 wy)) + fl(dz^2 wz)) with the integer squares converted exactly
 *   and every product and sum rounded once; wz, wy, wx are the SQUARED voxel spacings.  Computed as three separable
 *   passes (rows, then H, then D), which gives these bits because rounding is monotone; a minimum does not depend on
 *   its order, so a call repeats bit for bit.  A voxel that is set gets 0, a volume without a set voxel +inf everywhere.
 *   scratch: depgan_eval_edt_scratch_bytes(D, H, W) device bytes (0 for a volume outside the limits), 8-byte aligned
 *   like d2.  The host does not synchronise.
 * depgan_eval_surface_sums: over the n voxels with surf != 0, out_host = {their count, the maximum of d2 (0 when there
 *   is none; d2 >= 0), the sum of sqrt(d2) (a correctly rounded square root per voxel), the number of them whose d2 is
 *   +inf}.  One partial per block, then one block adds the partials in index order: the bits repeat from run to run.
 *   The two counts are integers held in doubles (exact below 2^53).  partial: depgan_eval_surface_sums_scratch_bytes(n)
 *   device bytes (0 unless 1 <= n < 2^31), 8-byte aligned.  Synchronises `stream`.
 * Status 1, nothing launched: a dimension below 1 or above 4096, D*H*W >= 2^31 (n outside 1 .. 2^31 - 1), a pointer
 *   NULL or misaligned, a weight that is not finite or not > 0, in_plane not 0 / 1, or an output or scratch range that
 *   overlaps an input range or another output. */
int depgan_eval_surface_mask(const unsigned char* set, int D, int H, int W, int in_plane, unsigned char* surf,
                             void* stream);
size_t depgan_eval_edt_scratch_bytes(int D, int H, int W);
int depgan_eval_edt_sq(const unsigned char* set, int D, int H, int W, double wz, double wy, double wx, double* d2,
                       void* scratch, void* stream);
size_t depgan_eval_surface_sums_scratch_bytes(long n);
int depgan_eval_surface_sums(const double* d2, const unsigned char* surf, long n, double* partial, double out_host[4],
                             void* stream);

/* ---- connected components (csrc/components.hip; evaluate.connected_components, lesion_detection) ----
 * Stateless; device pointers; enqueued on `stream`.  Volumes as above: (D, H, W) bytes with W contiguous, non-zero means
 * set, 1 <= D, H, W <= 4096 and D*H*W < 2^31.
 * depgan_eval_cc_label: labels[v] (int32) = 0 where set[v] is 0, else the number 1..N of v's component; N goes to
 *   n_out_host[0].  connectivity is scipy's rank, generate_binary_structure(3, connectivity): with in_plane 0, 1 is the 6
 *   face neighbours, 2 the 18 (faces and edges), 3 the 26; with in_plane 1 the neighbours lie in the slice only, 1 is 4
 *   and 2 and 3 are 8 (slices several times thicker than pixels, as depgan_eval_surface_mask's flag).  Canonical
 *   numbering: components are numbered in the order of their smallest linear index, which is scipy.ndimage.label's
 *   numbering, so every output is an integer with one right answer.  Label-equivalence union-find in six launches,
 *   whatever the content (no loop on the host that relaunches until nothing changes): run starts per row, unions over
 *   the backward half-neighbourhood by atomicMin on roots, compress, count roots per block, prefix sum, renumber.
 *   parent[x] <= x always holds, so every chase descends strictly and every retry of a union starts from a strictly
 *   smaller index: the loops are bounded by construction and no thread waits for another.  The root of a tree is its
 *   smallest index in whatever order the atomics land, so a call repeats bit for bit.
 *   scratch: depgan_eval_cc_scratch_bytes(D, H, W) device bytes (0 for a volume outside the limits), 8-byte aligned;
 *   labels 4-byte aligned.  Synchronises `stream`.
 * depgan_eval_cc_overlap: zeroes and fills two tables of n_comp ints over the n voxels of `labels`: size[k - 1] = the
 *   voxel count of component k, hits[k - 1] = the number of its voxels where other_or_null is non-zero (all 0 when it is
 *   NULL).  Integer atomic adds, one per run of equal labels in a wave: order-independent.  A label outside 1..n_comp is
 *   not counted.  n_comp = 0 is allowed and launches nothing (size and hits may then be NULL).  The host does not
 *   synchronise.
 * Status 1, nothing launched, every buffer untouched: a dimension below 1 or above 4096, D*H*W >= 2^31 (n outside
 *   1 .. 2^31 - 1), n_comp outside 0..n, connectivity not 1 / 2 / 3, in_plane not 0 / 1, a pointer NULL or misaligned, or
 *   an output or scratch range that overlaps an input range or another output. */
size_t depgan_eval_cc_scratch_bytes(int D, int H, int W);
int depgan_eval_cc_label(const unsigned char* set, int D, int H, int W, int connectivity, int in_plane, int* labels,
                         void* scratch, long long n_out_host[1], void* stream);
int depgan_eval_cc_overlap(const int* labels, const unsigned char* other_or_null, long n, int n_comp, int* size,
                           int* hits, void* stream);

/* ---- calibration of the class probabilities (csrc/calibration.hip; evaluate.calibration_census, fit_temperature,
 * apply_temperature) ----
 * Can the probabilities be believed?  Stateless; device pointers except the *_host outputs; enqueued on `stream`; no
 * global atomics.  Every double operation below is one correctly rounded operation in the stated order.
 * Shared conventions: prob is (npix, C) row-contiguous and 16-byte aligned, float32 for prob_kind 0 (predict) and float64
 * for prob_kind 1 (predict_mean, stats['mean']), C = 2..DEPGAN_MAX_HEAD_CLASSES.  lab is (npix) uint8 class codes,
 * ignore_label -1 (none) or 0..255, mask (npix) float32 or NULL.  Every element is converted to double first (exact), so
 * one rule serves both kinds.  A pixel is classified by the first statement that applies:
 *     mask[x] == 0 (mask given), or lab[x] == ignore_label      takes no part and is counted nowhere
 *     lab[x] >= C                                               n_bad; takes no part; its row is not read
 *     an element of its row is a NaN                            n_nan; takes no part
 *     otherwise                                                 TAKES PART; tc = lab[x] is its true class
 *   max(a, b) below is a < b ? b : a, so a NaN stays one.
 * depgan_eval_calibration_census: with
 *     b(v) = (int)min(max(v * bins, 0.0), bins - 1)              the product, the clamps and the truncation in double;
 *                                                                bins = 1..DEPGAN_CAL_MAX_BINS; v = k/bins sits in bin k
 *                                                                where the product is exact, 1.0 in bin bins - 1
 *     q(v) = (long long)rint(v * 2^DEPGAN_CAL_FIX_SHIFT)         the product is exact (a power of two), one rounding to
 *                                                                integer, ties to even; q(1) = 2^32
 *   over the pixels that take part:
 *     top label   conf = the first maximum of the row, pred = its index (depgan_eval_label_counts' tie rule, the lower
 *                 index wins); table 0, bin b(conf): count += 1, hits += (pred == tc), sum_q += q(conf)
 *     class k     (one against the rest) table 1 + k, bin b(p_k): count += 1, hits += (tc == k), sum_q += q(p_k)
 *     scalars     N += 1; n_floored += (r < eps), r = p_tc; n_nan and n_bad as above
 *     Brier       bs = 0; for c = 0..C-1: d = p_c - (c == tc ? 1.0 : 0.0); bs = bs + d * d.  The sum of bs.
 *     NLL         l = 0.0 - log(max(r, eps)), natural log in double.  The sum of l.  With eps = 0 nothing is floored and
 *                 r = 0 gives +inf: stated, not hidden.
 *   counts_out_host: (1 + C) * bins * 3 + 4 long long -- element ((j * bins + b) * 3 + f) is field f (0 count, 1 hits,
 *     2 sum_q) of bin b of table j, then {N, n_nan, n_bad, n_floored}.  sums_out_host: {Brier sum, NLL sum}.
 *   Everything in counts_out_host is an integer sum: it does not depend on the order of addition, repeats bit for bit,
 *   and a NumPy restatement gives the same bits (tests/calibration_ref.py).  A bin's mean confidence
 *   sum_q / (count * 2^32) is within 2^-33 of the mean of its values: |q(v) / 2^32 - v| <= 2^-33 per value (half a unit
 *   of the fixed point), the integer sum adds nothing, and a mean of errors is no larger than the largest.  sum_q is
 *   exact in 64 bits: |q| <= 2^32 for elements in [0, 1] and npix < 2^31.  Elements are expected in [0, 1]; any finite
 *   element is binned by the clamp, and |v| >= 2^31 or an infinite v leaves sum_q unspecified.
 *   The two double sums: a thread adds its pixels in grid-stride order, a fixed tree over the block's 256 threads, one
 *   partial per block, and one block adds the partials in index order.  The grid is a function of npix alone
 *   (min(ceil(npix / 1024), 1024) blocks), so the bits repeat from call to call.  No float atomics.
 *   Integers: a wave peels its distinct bins with ballots and adds once per distinct bin to the block's table in LDS
 *   (integer LDS adds); a block stores its table to scratch with plain stores; a finishing launch adds the tables.
 *   scratch: depgan_eval_calibration_scratch_bytes(npix, C, bins) device bytes (0 outside the limits), 8-byte aligned.
 *   Synchronises `stream` and copies the two tables to the host, as depgan_eval_surface_sums does.
 * depgan_eval_temperature_sums: over the pixels that take part, out_host = {N, sum L, sum L', sum L''} (N an integer
 *   held in a double) of the loss of the temperature-scaled probabilities at beta = 1 / T, eps in (0, 1):
 *     z_c = log(max(p_c, eps));  s_c = beta * z_c
 *     m = the maximum of s (folded left to right);  e_c = exp(s_c - m);  S = ((e_0 + e_1) + ...) in channel order
 *     lse = m + log(S);  pi_c = e_c / S
 *     A = sum_c pi_c * z_c;  B = sum_c pi_c * (z_c * z_c)        from 0.0, in channel order
 *     L = lse - s_tc;  L' = A - z_tc;  L'' = B - A * A
 *   L' and L'' are the first and second derivative of L in beta; L is convex in beta (L'' is a variance), which is why
 *   the entry is stated in beta and not in T.  The partial pattern of the two double sums above.  scratch:
 *   depgan_eval_calibration_scratch_bytes(npix, C, 1) bytes suffice.  Synchronises `stream`.
 * depgan_eval_apply_temperature: every pixel (no labels): z, s, m, S and lse as above with eps in [0, 1), then
 *     out_c = exp(s_c - lse)     in double, rounded once to the kind of prob
 *   out (the kind, shape and alignment of prob) may be prob itself or a disjoint range: a thread reads its whole row
 *   before it writes it.  Does not synchronise.
 * Status 1, nothing launched, every buffer untouched: npix outside 1 .. 2^31 - 1, C outside 2..DEPGAN_MAX_HEAD_CLASSES,
 *   bins outside 1..DEPGAN_CAL_MAX_BINS, prob_kind not 0 / 1, ignore_label outside -1..255, eps not in [0, 1) (not in
 *   (0, 1) for depgan_eval_temperature_sums), beta not finite or <= 0, a required pointer NULL, prob or out not 16-byte,
 *   mask not 4-byte or scratch not 8-byte aligned, scratch overlapping prob, lab or mask, or out overlapping prob
 *   without being prob. */
#define DEPGAN_CAL_MAX_BINS 64
#define DEPGAN_CAL_FIX_SHIFT 32
size_t depgan_eval_calibration_scratch_bytes(long npix, int C, int bins);
int depgan_eval_calibration_census(const void* prob, int prob_kind, int C, const unsigned char* lab, int ignore_label,
                                   const float* mask, long npix, int bins, double eps, void* scratch,
                                   long long* counts_out_host, double* sums_out_host, void* stream);
int depgan_eval_temperature_sums(const void* prob, int prob_kind, int C, const unsigned char* lab, int ignore_label,
                                 const float* mask, long npix, double beta, double eps, void* scratch,
                                 double out_host[4], void* stream);
int depgan_eval_apply_temperature(const void* prob, int prob_kind, int C, double beta, double eps, void* out, long npix,
                                  void* stream);

/* ---- parity-test surface: the tensors a training closure left behind ----
 * The step functions are piecewise linear in the ReLU signs and max-pool arg-maxes of the forward passes (GT:256-309
 * activations, GT:322-335 pools; the gradient penalty of GT:543-549 differentiates through them twice).  A parity
 * test that wants a bound EVERY evaluation must meet compares the gradients with a float64 restatement evaluated
 * under the very masks this library used; these two calls hand them out.
 * depgan_debug_capture(ctx, 1): from now on every critic closure keeps a copy of the post-ReLU activations of its
 *   interpolated ("mixed", GT:538 / 557) pass, which the penalty's second pass otherwise overwrites in place.
 * depgan_debug_tensor: copies one internal tensor to host memory as a dense (N, H, W, C) float32 array and reports
 *   its shape; host_dst == NULL only reports the shape.  Names (layer names as in the reference, GT:256-309, 319-339):
 *     "g/out/<layer>"   output of a generator trunk layer of the last generator pass: conv / FiLM block / deconv
 *                       (post-ReLU), "skip1..3" (the pooled tensor), "gen_segmentation" (tanh output)
 *     "g/u/<layer>"     BatchNorm output of a FiLM block's convolution (GT:402; kept by training passes only)
 *     "g/probs"         the (N, H, W, nc_out) probabilities the softmax of the last depgan_uresnet_* call wrote (a training
 *                       call: the phase-1 probabilities its loss and census were taken from); status 1 for nc_out = 1
 *     "g/heads"         the 14 noise-MLP head outputs, (N, 1, 1, 1024) in creation order (GT:363-395)
 *     "g/noise_a0", "g/noise_a1"   post-ReLU trunk activations of the noise MLP (GT:358-359), (N, 1, 1, 1024)
 *     "d/act/<layer>"   post-ReLU activations of critic layer dis_0a .. dis_8 of the last critic passes, 3*batch
 *                       sample slots [real | fake | mixed] (a generator pass leaves D_y2(fake_y2) in slots [0, batch) and
 *                       D_dem(attr) in [batch, 2 batch))
 *     "d/mixed/<layer>" the captured copy of the mixed pass (batch samples; needs depgan_debug_capture)
 *     "d/dz/<layer>"    gradient at the conv output of critic layer <layer> (after the ReLU mask), (3*batch, H_l, W_l,
 *                       Cout_l), slots as "d/act/"; a critic closure leaves g_z (upstream 1) in the mixed slots
 *     "d/pool/<layer>"  pooled output of a pooling critic layer (dis_0b, dis_1b, dis_3, dis_5), (3*batch, H_l/2, W_l/2,
 *                       Cout_l); after a critic closure the mixed slots hold the penalty's u gathered at the arg-max
 *                       (the mixed slots of "d/act/" of the non-pooling layers hold u as well).  Any other layer: status 1
 *     "d/in"            the critic input batch (3*batch, H, W, 1) [real | fake | mixed]; after a critic closure the mixed
 *                       slots hold u0 (GT:544-545); a generator pass does not write it
 *     "d/g0"            image gradients (2*batch, H, W, 1): after a critic closure only the first batch samples are
 *                       defined (d D(mixed) / d mixed); after a generator training closure D_y2's half, then D_dem's
 * Status 1 for an unknown name, a tensor that was not captured, or cap_floats too small. */
int depgan_debug_capture(depgan_ctx* ctx, int on);
int depgan_debug_tensor(depgan_ctx* ctx, const char* name, float* host_dst, long cap_floats, int shape[4]);

/* ---- generator forward with bf16 activation STORAGE (BASELINE config 4 as SURVEY 8d words it: bf16 weights AND bf16
 * activations, fp32 accumulate).  Opt-in, forward only; depgan_g_forward and every training closure keep fp32 storage.
 * Storage contract: element type bf16, NHWC, channel stride 1, strides counted in ELEMENTS.  A stored value is
 * RNE_bf16(v) of the fp32 epilogue result v (v_cvt_pk_bf16_f32) and nothing else: no truncation, no stochastic rounding.
 * Between the contraction and the store everything is fp32, in the order v = fma(acc, scale, bias * scale + shift),
 * FiLM (v * mul + add, two roundings), ReLU, + residual (read as bf16, widened exactly).  A 2x2 max-pool is the max of
 * the stored values (RNE is monotone: the same as rounding the fp32 max).  The network input x and the output stay fp32;
 * weights are the context's bf16 panels; fp32 masters, Adam, the noise MLP and its FiLM vectors stay fp32.
 * depgan_g_forward_bf16s: contract of depgan_g_forward (n in [1, batch], phase 0, enqueued on the context's stream).
 *   Needs a context created with bf16_mfma = 1 (hence bf16_weights = 1, nc_out = 1); any other context gets status 3
 *   and a message naming the settings, before any launch.  The bf16 buffers (one per generator layer output, concat
 *   buffers shared) are allocated by the first call, kept, and freed by depgan_destroy.
 *   On an inference context (bf16_mfma = 1, nc_out = K >= 2) the same walk, bit for bit up to gen_17, ends in
 *   depgan_op_head_softmax_k_bf16s of the stored gen_17 and out_dev is (n, H, W, K) class probabilities; depgan_g_forward
 *   on such a context (bf16 pipe, fp32 storage, the direct 1x1 head, its own softmax launch) is the same-context A/B
 *   partner.
 * depgan_debug_tensor_bf16s: "g/out/<layer>" as depgan_debug_tensor resolves it, from the bf16 buffers of the last
 *   depgan_g_forward_bf16s, widened to fp32 (exact): every conv / FiLM / deconv / pool layer, gen_17 included.
 *   ("g/out/gen_segmentation" is the call's own fp32 output and has no bf16 buffer: status 1.) */
int depgan_g_forward_bf16s(depgan_ctx* ctx, const float* x_dev, const float* z_dev, float* out_dev, int n);
int depgan_debug_tensor_bf16s(depgan_ctx* ctx, const char* name, float* host_dst, long cap_floats, int shape[4]);

/* ---- bf16 activation storage for the FORWARD-ONLY generator passes of the training closures.  Opt-in, default 0.
 * Of the 21 generator forwards of one generator iteration of the reference schedule (5 + 5 critic updates, 10
 * evaluations, 1 update) 20 keep nothing for a backward pass: the critic updates do not differentiate G (GT:549, 568)
 * and netG_no_update is the best-of-k evaluation (GT:868-877).  With storage = 1 those passes -- the generator pass
 * inside depgan_critic_grads / depgan_critic_step / depgan_g_eval / depgan_g_eval_multi and both critic loops and the
 * k evaluations of depgan_gen_iteration -- run the forward of depgan_g_forward_bf16s (same storage contract) with
 * gen_segmentation fused into gen_17's epilogue, so that gen_17 is neither stored nor read back
 * (DEPGAN_BF16S_HEAD_FUSED=0, read by depgan_create, keeps the two launches: A/B).  The generator UPDATE
 * (depgan_g_grads, depgan_g_step, the update closing depgan_gen_iteration) keeps the fp32-storage forward and the
 * existing backward unless depgan_set_g_update_storage(ctx, 1) puts it on the same storage; depgan_g_forward,
 * depgan_g_forward_bf16s and the DEP-UResNet entries are not affected.  With
 * storage = 0 every path computes the bits it computed before this option existed.
 * Consequence to know (without depgan_set_g_update_storage): with storage = 1 netG_no_update(z) evaluates the bf16-storage generator and netG_train(z)
 * reports the fp32-storage one, so the two no longer return identical scalars for the same noise, and the noise
 * best-of-k picks is the arg-min under the bf16-storage forward.  In a data-parallel job every rank must use the same
 * value (the mode changes no collective; the arg-min is formed from all-reduced pieces, so the ranks agree anyway).
 * depgan_set_fwd_only_storage: 0 = fp32 (default), 1 = bf16.  1 is refused with status 3 and a message naming the
 *   cause, before any launch, for whatever depgan_g_forward_bf16s refuses (no bf16_mfma, nc_out != 1, a layer without
 *   a bf16 plan); any other value is status 1.  The bf16 buffers are those of depgan_g_forward_bf16s: allocated by the
 *   first pass that needs them and kept -- 58 MB per sample of batch at 256 x 256 on top of the fp32 set.
 * Debug surface with storage = 1: "g/out/gen_segmentation" of depgan_debug_tensor is the generator output of the last
 *   pass whichever storage wrote it; the other fp32 "g/out/<layer>" names describe the last fp32-storage pass.  The bf16
 *   buffers of the last forward-only pass are read with depgan_debug_tensor_bf16s; "g/out/gen_17" is stored by those
 *   passes only while depgan_debug_capture is on -- after a pass that skipped the store it is refused with status 1
 *   and a message that says so (never stale data); every other layer stays readable. */
int depgan_set_fwd_only_storage(depgan_ctx* ctx, int storage);
int depgan_get_fwd_only_storage(depgan_ctx* ctx);

/* ---- bf16 activation storage for the generator UPDATE.  Opt-in, default 0, independent of
 * depgan_set_fwd_only_storage.  With storage = 1 the training pass of g_eval -- depgan_g_grads, depgan_g_step and the
 * update closing depgan_gen_iteration -- runs the forward of depgan_g_forward_bf16s (same storage contract, same attr
 * bits as that call and as the forward-only passes of depgan_set_fwd_only_storage) and a backward that reads every
 * generator activation from the bf16 buffers: weight-gradient operands staged from bf16 memory, ReLU masks `stored > 0`,
 * pool arg-max on the stored values.  Gradients (dout / din / du, the gradient arena, the data-parallel all-reduce)
 * stay fp32; no fp32 copy of a generator activation is written.  The forward additionally keeps, per FiLM layer,
 * u = RNE_bf16 of the pre-FiLM value (FiLM itself is computed from the unrounded fp32 value, so the output bits do not
 * change) and the ReLU decision its epilogue took, one bit per element; the FiLM backward uses that stored decision and
 * never re-derives it from the rounded u.  The gradient is the backward of the stored graph with each storage rounding
 * treated as the identity (straight-through).  With both modes on, netG_no_update(z) and the pre-update scalars of
 * netG_train(z) are the same bits again.  With storage = 0 every path computes the bits it computed before.
 * depgan_set_g_update_storage: 0 = fp32 (default), 1 = bf16; refusals as depgan_set_fwd_only_storage.  Extra memory, on
 *   top of the bf16 buffers of depgan_g_forward_bf16s: the u buffers, 7.2 M bf16 elements = 14.4 MB per sample of batch
 *   at 256 x 256, plus 0.9 MB per sample of decision bits; allocated by the first update in the mode and kept.
 * depgan_debug_tensor_bf16s additionally serves "g/u/<film layer>" (the stored u, widened) after a training forward in
 *   the mode; before one it is refused with status 1.
 * depgan_debug_film_decision_bf16s: the stored decisions of a FiLM layer ("gen_2", ...) as one byte (0 / 1) per element,
 *   (N, H, W, C); host_dst == NULL only reports the shape; status 1 before a training forward in the mode. */
int depgan_set_g_update_storage(depgan_ctx* ctx, int storage);
int depgan_get_g_update_storage(depgan_ctx* ctx);

/* ---- the critics' 16-channel 5x5 layers on the bf16 matrix pipe.  Opt-in, default 0.
 * A bf16_mfma context runs every convolution with Cout % 32 == 0 on v_mfma_f32_32x32x16_bf16; the launches of the
 * critics whose output-channel count is 16 stayed on the fp32 pipe (igemm_conv_kernel<16,5,16,25,..>).  With pipe = 1
 * they run on igemm_bf16_n16_kernel (csrc/igemm_bf16.hip, v_mfma_f32_16x16x32_bf16) under the operand contract of the
 * other bf16 launches: the fp32 activation view is rounded to bf16 (RNE) while it is staged, the weights are the
 * context's bf16-valued weights, accumulation and the whole epilogue are fp32, the K order is fixed (chunk, then tap: the
 * bits repeat from run to run and do not depend on how many samples share the launch).  The launches that move, in both
 * critics: dis_0b forward (bias, ReLU, fused pool), the penalty's u-forward of dis_0b (mask) and dis_0b backward-data
 * (5x5, 16 -> 16 at full resolution), and dis_1a backward-data (5x5, 32 -> 16 at half resolution) -- in depgan_d_forward,
 * depgan_critic_grads / depgan_critic_step, the critic passes of depgan_g_eval / depgan_g_eval_multi / depgan_g_grads /
 * depgan_g_step, and depgan_gen_iteration.  Not touched: the weight gradients (already on the bf16 pipe), dis_0a (one
 * input channel) and its backward-data (one output channel), every other layer, the generator.  With pipe = 0 every path
 * computes the bits it computed before this option existed; switching needs no other call and allocates nothing (both
 * panels of the four launches are planned and packed by every bf16_mfma context, a few KB).
 * depgan_set_critic16_pipe: 0 = fp32 (default), 1 = bf16; any other value is status 1; 1 on a context without
 *   bf16_mfma (or without critics) is status 3 with a message naming the setting, before any launch.
 * In a data-parallel job every rank must use the same value (the mode changes no collective, but the ranks would
 * otherwise average gradients of two different critics' arithmetic). */
int depgan_set_critic16_pipe(depgan_ctx* ctx, int pipe);
int depgan_get_critic16_pipe(depgan_ctx* ctx);
int depgan_debug_film_decision_bf16s(depgan_ctx* ctx, const char* layer, unsigned char* host_dst, long cap_bytes,
                                     int shape[4]);

/* Operators of the update on bf16 storage: conventions of the operators below (explicit element strides, stream last,
 * status 1 for null / non-positive arguments before any HIP call, 3 for shapes the kernels do not cover).
 * depgan_op_conv2d_film_train_bf16s: depgan_op_conv2d_bf16s (KS = 3, FiLM required) that also stores u_out = RNE_bf16 of
 *   the pre-FiLM value, dense (B, H, W, Cout) bf16, and dec_bits: bit (c & 7) of byte [pixel (Cout / 8) + c / 8] =
 *   (FiLM result > 0), B H W Cout / 8 bytes, 4-byte aligned.  `out` has the bits of depgan_op_conv2d_bf16s.
 * depgan_op_conv2d_wgrad_bf16s: dw[tap][ci][co] (oi = 1: [tap][co][ci]) = sum x[pixel + tap][ci] dy[pixel][co], x a bf16
 *   view staged as it is, dy an fp32 view rounded to bf16 (RNE) while staged; KS in {1, 3}, Cin % 8 == 0, Cout % 4 == 0;
 *   colsum (optional, Cout floats) = column sums of the unrounded dy.  Same K order as depgan_op_conv2d_wgrad_bf16:
 *   bit-equal to it on the widened operand.
 * depgan_op_conv2d_bwd_data_bf16s: dx = (mask > 0) ? bwd_data(dy, w) + res : 0 with dy fp32 (rounded while staged), res
 *   fp32 (optional), mask a bf16 view (optional), dx fp32, all (H, W) views of Cin channels except dy (Cout channels).
 *   deconv = 0: 3x3, w HWIO (Cin, Cout).  deconv = 1: dy is the (2H, 2W) upstream gradient of Conv2DTranspose(2x2,
 *   stride 2) with (kh, kw, Cout, Cin) weights, contracted as one 1x1 convolution over its four pixel grids.
 * depgan_op_unpool_mask_bf16s: depgan_op_unpool_mask with a bf16 `a`; C % 8 == 0.  The arg-max of a window is its FIRST
 *   maximum in the order (0,0), (0,1), (1,0), (1,1), as in the fp32 kernel.
 * depgan_op_film_bwd_bf16s: dv = dec ? dr : 0; du = dv * fmul; dmul[b][c] = sum_p dv * u; dadd[b][c] = sum_p dv; u dense
 *   bf16 (B, HW, C), dec_bits as above, dr / du dense fp32; C % 8 == 0, C <= 256.
 * depgan_op_head_bwd_bf16s: backward = 0: out[c] = sum_p dpre[p] a[p ld + c]; backward = 1: out[p][c] = (a > 0) ?
 *   dpre[p] w[c] : 0; a bf16 with row stride ld. */
int depgan_op_conv2d_film_train_bf16s(const void* in, long isB, long isY, long isX, const float* w_hwio, const float* bias,
                                      const float* scale, const float* shift, const float* film_mul, const float* film_add,
                                      int film_ld, const void* res, long rsB, long rsY, long rsX, void* out, long osB,
                                      long osY, long osX, void* u_out, unsigned char* dec_bits, int B, int H, int W, int Cin,
                                      int Cout, int relu, void* hip_stream);
int depgan_op_conv2d_wgrad_bf16s(const void* x, long xsB, long xsY, long xsX, const float* dy, long dsB, long dsY, long dsX,
                                 float* dw, float* colsum, int B, int H, int W, int Cin, int Cout, int KS, int oi,
                                 void* hip_stream);
int depgan_op_conv2d_bwd_data_bf16s(const float* dy, long dsB, long dsY, long dsX, const float* w, const float* res,
                                    long rsB, long rsY, long rsX, const void* mask, long msB, long msY, long msX, float* dx,
                                    long osB, long osY, long osX, int B, int H, int W, int Cin, int Cout, int deconv,
                                    void* hip_stream);
int depgan_op_unpool_mask_bf16s(const float* dpool, long dsB, long dsY, long dsX, const void* a, long asB, long asY, long asX,
                                const float* skip, long ssB, long ssY, long ssX, float* out, long osB, long osY, long osX,
                                int B, int Ho, int Wo, int C, void* hip_stream);
int depgan_op_film_bwd_bf16s(const float* dr, const void* u, const unsigned char* dec_bits, const float* fmul, int film_ld,
                             float* du, float* dmul, float* dadd, int B, long HW, int C, void* hip_stream);
int depgan_op_head_bwd_bf16s(int backward, const void* a, long ld, const float* w, const float* dpre, float* out, long P,
                             int C, void* hip_stream);

/* Operators of that path.  bf16 tensors are void* device pointers with explicit view strides (sample, row, pixel) in
 * ELEMENTS; every bf16 view must be 16-byte aligned (pointer, strides multiples of 8).  Status 1 for null / non-positive
 * arguments (checked before any HIP call), 3 for shapes the kernels do not cover.
 * depgan_op_conv2d_bf16s: KS in {1, 3}, Cin % 8 == 0, Cout % 32 == 0; HWIO fp32 weights are packed (rounded to bf16)
 *   inside; bias, scale + shift, FiLM (mul, add: [B][ld] fp32), residual view `res` and the dense (B, H/2, W/2, Cout)
 *   bf16 max-pool output `pool` are optional (NULL); `pool` needs even H and W.
 * depgan_op_deconv2x2_bf16s: Conv2DTranspose(2x2, stride 2) with (kh, kw, Cout, Cin) fp32 weights as ONE grouped launch
 *   of the same kernel; `out` is the (2H, 2W) view.
 * depgan_op_edge_conv_bf16s: 3x3, Cin in {1, 2}, Cout in {8, 16, 24, 32}; dense fp32 input (B, H, W, Cin), bf16 output.
 * depgan_op_head_bf16s: out[p] = act(sum_c a[p][c] w[c] + b[0]), dense bf16 a (P, C), fp32 out; act = tanh if tanh_act.
 * depgan_op_conv2d_head_bf16s: depgan_op_conv2d_bf16s with that head fused into the epilogue (KS = 3, Cout = 32; status
 *   3 otherwise): head_out (B, H, W) dense fp32 is computed from the STORED (rounded) values in depgan_op_head_bf16s's
 *   arithmetic and order, so it equals the two calls bit for bit; with skip_out the stores of `out` are not issued.
 * depgan_op_head_softmax_bf16s: the DEP-UResNet's head.  z[p][k] = sum_c a[p ld + c] w[c][k] + b[k] for k = 0..3, bf16 a
 *   with row stride ld >= C elements (ld % 8 == 0), w (C, 4) fp32 (HWIO of a 1x1 kernel), each column in
 *   depgan_op_head_bf16s's arithmetic and order; probs[p] = softmax(z[p]) in depgan_op_softmax_ce4's arithmetic, dense
 *   fp32 (P, 4); `logits` (P, 4) receives z where it is not NULL.  a, w, probs and logits 16-byte aligned; C / 8 a power
 *   of two <= 64.  It is depgan_op_head_softmax_k_bf16s with K = 4.
 * depgan_op_head_softmax_k_bf16s: that head for K = 2..DEPGAN_MAX_HEAD_CLASSES classes: w (C, K), b (K), probs and
 *   logits dense (P, K); each logit column in depgan_op_head_bf16s's arithmetic and order, the softmax in
 *   depgan_op_softmax_ce's arithmetic for K classes.  a 16-byte aligned; w, probs and logits 16-byte aligned where
 *   K % 4 == 0, else 4-byte. */
int depgan_op_conv2d_bf16s(const void* in, long isB, long isY, long isX, const float* w_hwio, const float* bias,
                           const float* scale, const float* shift, const float* film_mul, const float* film_add,
                           int film_ld, const void* res, long rsB, long rsY, long rsX, void* out, long osB, long osY,
                           long osX, void* pool, int B, int H, int W, int Cin, int Cout, int KS, int relu,
                           void* hip_stream);
int depgan_op_conv2d_head_bf16s(const void* in, long isB, long isY, long isX, const float* w_hwio, const float* bias,
                                const float* scale, const float* shift, const float* film_mul, const float* film_add,
                                int film_ld, const void* res, long rsB, long rsY, long rsX, void* out, long osB,
                                long osY, long osX, void* pool, int B, int H, int W, int Cin, int Cout, int KS, int relu,
                                const float* head_w, const float* head_b, float* head_out, int tanh_act, int skip_out,
                                void* hip_stream);
int depgan_op_deconv2x2_bf16s(const void* in, long isB, long isY, long isX, const float* w_hwoi, const float* bias,
                              const float* scale, const float* shift, void* out, long osB, long osY, long osX, int B,
                              int H, int W, int Cin, int Cout, int relu, void* hip_stream);
int depgan_op_edge_conv_bf16s(const float* in, const float* w_hwio, const float* bias, const float* scale,
                              const float* shift, void* out, long osB, long osY, long osX, int B, int H, int W, int Cin,
                              int Cout, int relu, void* hip_stream);
int depgan_op_head_bf16s(const void* a, const float* w, const float* b, float* out, long P, int C, int tanh_act,
                         void* hip_stream);
int depgan_op_head_softmax_bf16s(const void* a, long ld, const float* w, const float* b, float* probs,
                                 float* logits_or_null, long P, int C, void* hip_stream);
int depgan_op_head_softmax_k_bf16s(const void* a, long ld, const float* w, const float* b, float* probs,
                                   float* logits_or_null, long P, int C, int K, void* hip_stream);

/* ---- single operators (unit-test surface; device pointers) ---- */
/* path: 0 auto, 1 fp32 MFMA implicit GEMM, 2 direct, 3 bf16 MFMA implicit GEMM (both operands rounded to bf16, RNE),
 * 4 / 5: fp32 operands split into 2 / 3 bf16 terms, 3 / 6 products on the bf16 pipe (depgan_config.f32_split = 3 / 6),
 * 6: fp32 MFMA with 8-channel chunks, workgroup tiles (large 3x3 launches with more than 64 input channels),
 * 7: the wave-private form of 6 (csrc/igemm_wp.hip: large 3x3 launches with Cin <= 64; bit-identical to 6),
 * 8: Winograd F(2x2,3x3) on the fp32 matrix pipe (csrc/igemm_wino.hip: 3x3, Cin % 8 == 0, Cout % 32 == 0, even H, W),
 * 9: the weight-stationary, wave-private 5x5 form of 1 (csrc/igemm_wp.hip: 5x5, Cin and Cout in {16, 32}, no fused
 *    head; any size; bit-identical to 1; status 1 for KS != 5, status 3 for everything else it does not cover),
 * 10: the 16-output-channel 5x5 form of 3 (igemm_bf16_n16_kernel: 5x5, output channels of the launch -- Cout, or Cin
 *    for backward-data -- a multiple of 16, input channels >= 8 and a multiple of 4; status 1 for KS != 5, null operands
 *    or a fused head, status 3 for every other shape it does not cover; all decided before any HIP call) */
int depgan_op_conv2d(const float* in, const float* w_hwio, const float* bias, float* out, int B, int H, int W,
                     int Cin, int Cout, int KS, int relu, int path, void* hip_stream);
int depgan_op_conv2d_bwd_data(const float* dy, const float* w_hwio, float* dx, int B, int H, int W, int Cin,
                              int Cout, int KS, int path, void* hip_stream);
int depgan_op_conv2d_wgrad(const float* x, const float* dy, float* dw_hwio, int B, int H, int W, int Cin, int Cout,
                           int KS, void* hip_stream);
/* the same contraction on the bf16 matrix pipe (depgan_config.bf16_mfma: both operands rounded to bf16, RNE, while
 * staged; fp32 accumulation).  KS in {1, 3, 5}, Cin >= 8, Cin and Cout multiples of 4; status 3 otherwise. */
int depgan_op_conv2d_wgrad_bf16(const float* x, const float* dy, float* dw_hwio, int B, int H, int W, int Cin,
                                int Cout, int KS, void* hip_stream);

/* diagnostics: MFMA conv with per-workgroup phase stamps (16 x u64 per workgroup: start, after first prefetch
 * issue, stage-0 ready, stage-1 ready, MFMAs done, end, realtime ticks, HW_ID) */
int depgan_op_conv2d_stamps(const float* in, const float* w_hwio, float* out, int B, int H, int W, int Cin, int Cout,
                            int KS, unsigned long long* stamps, int reps, void* hip_stream);
int depgan_op_maxpool(const float* in, float* out, int B, int Ho, int Wo, int C, void* hip_stream);
/* Forward of the 2x2 / stride-2 transposed convolution (Conv2DTranspose, GT:308) on the fused four-tap kernel:
 * out[b][2i+di][2j+dj][co] = act((sum_ci in[b][i][j][ci] w[di][dj][co][ci] + bias[co]) * scale[co] + shift[co]).
 * w_hwoi is the Keras kernel (2, 2, Cout, Cin); bias / scale+shift may be null; out is dense (B, 2H, 2W, Cout).
 * Status 3 when the kernel does not cover the shape (Cin in {64, 96, 128}, Cout % 32 == 0, H and W
 * powers of two, W >= 8, B H W % 32 == 0). */
int depgan_op_deconv2x2(const float* in, const float* w_hwoi, const float* bias, const float* scale,
                        const float* shift, float* out, int B, int H, int W, int Cin, int Cout, int relu,
                        void* hip_stream);
/* The same launch with the output given as a view: out points at sample 0, row 0, column 0, channel 0 of the (2H, 2W)
 * output grid and osB / osY / osX are its float strides between samples, rows and pixels -- the channel slice of a concat
 * buffer the model stores into (osX > Cout).  Status 3 when the kernel does not cover the launch: the shapes above, an
 * out that is not 16-byte aligned, a stride that is no multiple of 4, or B * osB above 2^31 - 1 (the kernel addresses the
 * output with 32-bit float offsets).  A refusal launches and writes nothing. */
int depgan_op_deconv2x2_ex(const float* in, const float* w_hwoi, const float* bias, const float* scale,
                           const float* shift, float* out, long osB, long osY, long osX, int B, int H, int W, int Cin,
                           int Cout, int relu, void* hip_stream);
/* Host only (no launch, no allocation): the geometry the launcher of the fused forward kernel takes for a dense launch of
 * this shape on the current device, from the function the launcher itself calls.
 * out = {32-pixel tiles, gridDim.x, gridDim.y, workgroups per CU the launcher counts on}: gridDim.x =
 * min(CUs * workgroups per CU / gridDim.y, tiles), and workgroup x walks the tiles x, x + gridDim.x, ...
 * Status 3 for a shape the kernel does not cover, status 1 for a null `out` or a non-positive size.  A refusal writes
 * nothing. */
int depgan_debug_deconv_fwd_plan(int B, int H, int W, int Cin, int Cout, long out[4]);

/* Weight gradient of the same layer on the fused kernel (four taps + the column sums of dout in one launch):
 * dw_hwoi[di][dj][co][ci] = sum_p dout[b][2i+di][2j+dj][co] in[b][i][j][ci]; colsum[co] (optional) = sum of dout over
 * all output pixels.  Status 3 when not covered (Cin = Cout in {64, 96, 128}, H and W powers of two). */
int depgan_op_deconv2x2_wgrad(const float* in, const float* dout, float* dw_hwoi, float* colsum, int B, int H, int W,
                              int Cin, int Cout, void* hip_stream);

/* The fp32 convolution kernels as the model launches them: every operand an NHWC view with the float strides
 * (sB, sY, sX) and channel stride 1, and the whole fused epilogue, applied to the raw contraction acc in this order:
 *   v = (acc + bias[co]) * scale[co] + shift[co];  out_pre = v;  v = v * film_mul[b][co] + film_add[b][co];
 *   v = max(v, 0) if relu;  v += res;  v = mask > 0 ? v : 0;  out = accumulate ? out + v : v;
 *   pool (view of (H/2, W/2) pixels) = 2x2 / stride-2 maximum of out;
 *   head_out[b][y][x] = act(sum_co out[co] head_w[co] + head_b[0]), act = tanh when head_tanh (dense (B, H, W));
 *   head_skip_out: out itself is not stored.
 * Optional operands are NULL (their strides are then ignored); scale / shift and film_mul / film_add come in pairs;
 * film_mul / film_add are rows of film_ld floats per sample.  w_hwio is (KS, KS, Cin, Cout); bwd = 1 is the
 * backward-data form: `in` has Cout channels, `out` (and the epilogue operands) Cin.  path as in depgan_op_conv2d:
 * 1 MFMA, 2 direct, 3 bf16 pipe, 4 / 5 split, 6 8-channel chunks, 7 wave-private, 8 Winograd, 9 weight-stationary 5x5, 10 bf16 pipe with 16-channel tiles (5x5).  Status 1 for null or
 * non-positive arguments (before any HIP call) and whatever the launcher's argument checks refuse, 3 for what the kernel
 * of that path does not cover; nothing is written then. */
int depgan_op_conv2d_fused(const float* in, long isB, long isY, long isX, const float* w_hwio, const float* bias,
                           const float* scale, const float* shift, const float* film_mul, const float* film_add,
                           int film_ld, float* out, long osB, long osY, long osX, float* out_pre, long psB, long psY,
                           long psX, const float* res, long rsB, long rsY, long rsX, const float* mask, long msB,
                           long msY, long msX, float* pool, long qsB, long qsY, long qsX, const float* head_w,
                           const float* head_b, float* head_out, int head_tanh, int head_skip_out, int B, int H, int W,
                           int Cin, int Cout, int KS, int relu, int accumulate, int path, int bwd, void* hip_stream);
/* The Winograd 3x3 kernel (path 8 above) with a gathered K axis, the launch form ConvArgs::cpt describes: the Cin input
 * channels are `runs` (1 ... 4) equal runs of whole 8-channel chunks, run t read at in + run_off[t] floats with the
 * strides of `in` (run_off: HOST array of `runs` offsets, multiples of 4).  w_hwio (3, 3, Cin, Cout) with the runs in
 * order along Cin; bias optional.  Status 1 for bad arguments, 3 for what the kernel does not cover. */
int depgan_op_conv3x3_wino_gathered(const float* in, long isB, long isY, long isX, const long* run_off, int runs,
                                    const float* w_hwio, const float* bias, float* out, long osB, long osY, long osX,
                                    int B, int H, int W, int Cin, int Cout, void* hip_stream);
/* Epilogue classes of the Winograd 3x3 kernel: for each flag set of the fused epilogue that the model launches, an
 * instantiation that carries the flags as compile-time constants (same statements, same bits as the generic kernel,
 * fewer instructions per work item).  A flag set is a mask of DEPGAN_EPF_* -- which optional operands of
 * depgan_op_conv2d_fused are present, in its order: bias, scale/shift, film_mul/film_add, relu, out_pre, res, mask, pool,
 * accumulate, head_out.
 * depgan_set_epilogue_classes(on): process-wide A/B switch, 1 (default) = launches take the class of their flag set,
 *   0 = every launch takes the generic kernel; any other value is status 1.  The environment variable
 *   DEPGAN_EPI_CLASSES=0 sets the initial state to 0.  depgan_get_epilogue_classes() returns the state.
 * depgan_wino_epilogue_class(flags, form): host only, no HIP call: the class id a launch with this flag set takes.
 *   form 0: the 8-row kernel (wino_conv_kernel<1,...>), 1: the fused-head kernel, 2: the 16-row kernel without head,
 *   3: gathered K.  0 = the generic kernel: sets outside the table, forms 2 and 3, everything while the switch is off.
 *   -1 (and a message) for flags outside DEPGAN_EPF_ALL or a form outside 0 ... 3.
 * depgan_op_conv3x3_wino_kernel_name: the kernel instantiation (as rocprofv3 prints it, e.g. "wino_conv_kernel<1,true,1>":
 *   8-row tiles, persistent grid, class 1) that depgan_op_conv2d_fused on path 8 launches for a (B, H, W, Cin) -> Cout
 *   convolution with this flag set on the current device, from the same selection function the launcher calls; written
 *   to buf (cap bytes, NUL-terminated).  Launches nothing.  Status 1 for bad arguments, 3 for a shape the kernel does
 *   not cover.
 * The 5x5 kernels (paths 1 and 9 with KS = 5: igemm_ws5_kernel and the persistent igemm_conv_kernel<.,5,.,25,true>) have
 * classes too, selected INSIDE the kernel: the kernel's name, grid and LDS size are the same for every class, and the
 * same switch sends every launch through the run-time-flag body.
 * depgan_conv5_epilogue_class(flags): host only, no HIP call: 1 {bias, relu}, 2 {bias, relu, pool}, 3 {mask}, 4 {} (no
 *   flag); 0 = the run-time-flag body: every other set, and everything while the switch is off.  -1 (and a message) for
 *   flags outside DEPGAN_EPF_ALL. */
#define DEPGAN_EPF_BIAS 1
#define DEPGAN_EPF_AFFINE 2
#define DEPGAN_EPF_FILM 4
#define DEPGAN_EPF_RELU 8
#define DEPGAN_EPF_PRE 16
#define DEPGAN_EPF_RES 32
#define DEPGAN_EPF_MASK 64
#define DEPGAN_EPF_POOL 128
#define DEPGAN_EPF_ACCUM 256
#define DEPGAN_EPF_HEAD 512
#define DEPGAN_EPF_ALL 1023
int depgan_set_epilogue_classes(int on);
int depgan_get_epilogue_classes(void);
int depgan_wino_epilogue_class(unsigned flags, int form);
int depgan_conv5_epilogue_class(unsigned flags);
int depgan_op_conv3x3_wino_kernel_name(unsigned flags, int B, int H, int W, int Cin, int Cout, char* buf, int cap);
/* The 2x2 / stride-2 transposed convolution on the implicit-GEMM kernels, w_hwoi the Keras kernel (2, 2, Cout, Cin).
 * form 0: forward as ONE grouped launch of four 1x1 convolutions: in (B, H, W, Cin) -> out (B, 2H, 2W, Cout), with
 *         bias / scale+shift / relu; mask must be NULL.
 * form 1: backward-data as ONE 1x1 convolution whose K axis gathers the four pixel grids of the upstream gradient:
 *         in = dOut (B, 2H, 2W, Cout) -> out = dIn (B, H, W, Cin), times (mask > 0) when mask (B, H, W, Cin) is given.
 * form 2: the same as four accumulating 1x1 launches, one per pixel grid.
 * path 1 (fp32 MFMA), 3 (bf16 pipe) or 8 (Winograd: no 1x1 form, status 3). */
int depgan_op_deconv2x2_igemm(int form, const float* in, long isB, long isY, long isX, const float* w_hwoi,
                              const float* bias, const float* scale, const float* shift, float* out, long osB, long osY,
                              long osX, const float* mask, long msB, long msY, long msX, int B, int H, int W, int Cin,
                              int Cout, int relu, int path, void* hip_stream);
/* Weight gradient as the model runs it (slab kernel, then the finishing launch): dw[tap][ci][co] (oi = 1:
 * [tap][co][ci]) (+)= scale[co] * g, raw (optional) = g, g[tap][ci][co] = sum over pixels of x (shifted by the tap) dy;
 * x and dy strided views.  Column sums of dy over the samples b < colB when colout or colraw is given:
 * colout[co] = colscale[co] (or 1) * sum, colraw[co] = sum; without them colB must be 0.  bf16 = 1: the contraction on
 * the bf16 matrix pipe (status 3 where wgrad_bf16.hip does not cover the shape). */
int depgan_op_conv2d_wgrad_ex(const float* x, long xsB, long xsY, long xsX, const float* dy, long dsB, long dsY,
                              long dsX, const float* scale, float* dw, float* raw, int accumulate, int oi, int colB,
                              const float* colscale, float* colout, float* colraw, int B, int H, int W, int Cin,
                              int Cout, int KS, int bf16, void* hip_stream);
/* Host only (no launch, no allocation): the launch plan a weight-gradient launcher computes for a shape on the current
 * device, from the same chunking function the launcher calls.  kernel: 0 fp32 MFMA (wgrad.hip), 1 edge layers
 * (direct.hip: Cin < 8 or channels that are no multiple of 4), 2 bf16 pipe with fp32 staging (wgrad_bf16.hip), 3 bf16 pipe
 * with bf16 staging (wgrad_bf16s.hip), 4 transposed convolution (deconv_wgrad.hip; KS is ignored).
 * out = {pixel tiles, tiles per workgroup, chunks (= partial slabs), gridDim.y}; kernel 4: {k-steps of 4 pixels, k-steps
 * per workgroup, workgroups along x, gridDim.y}.  A shape the launcher refuses returns the launcher's status; a null
 * `out`, a non-positive size or an unknown `kernel` status 1. */
int depgan_debug_wgrad_plan(int kernel, int KS, int B, int H, int W, int Cin, int Cout, int out[4]);
/* Host only (no launch, no allocation): the slab kernel every weight gradient of the library takes for a shape -- the
 * model's and the depgan_op_conv2d_wgrad* entries' -- with bf16_pipe = 1 where the contraction may run on the bf16 matrix
 * pipe and x_bf16 = 1 where the activation operand lies in bf16 memory.  With mfma = Cin % 4 == 0 && Cout % 4 == 0 &&
 * Cin >= 8: x_bf16 takes kernel 3 or is refused with status 3 (the storage types are not mixed); else bf16_pipe && mfma
 * takes kernel 2 where wgrad_bf16.hip covers the shape; else mfma takes kernel 0; else kernel 1.
 * out = {kernel (the numbering above), chunks (out[2] of depgan_debug_wgrad_plan for that kernel), floats of the slab
 * workspace (chunks * KS * KS * Cin * Cout), partial column-sum rows of Cout floats the launch writes when column sums
 * are asked for (chunks; 0 for kernel 1, whose column sums are a streaming pass of their own)}.  A shape the chosen
 * launcher refuses returns the launcher's status; a null `out`, a non-positive size or a flag that is not 0 or 1
 * status 1.  A refusal writes nothing. */
int depgan_debug_wgrad_choice(int KS, int B, int H, int W, int Cin, int Cout, int bf16_pipe, int x_bf16, long out[4]);
/* Host only (no launch, no allocation): the kernel and the launch geometry the model takes for one convolution -- the
 * layer planned as a context in the given mode plans it (f32_split 0, 3 or 6; bf16_mfma and winograd 0 or 1; planN the
 * batch the layer is planned for, 0 where the plan does not depend on it), launched at batch B with the operands that
 * epilogue_flags (DEPGAN_EPF_* bits) names.  groups = 4: the grouped launch of a transposed convolution's four taps;
 * runs > 0: gathered K, Cin in `runs` runs of whole chunks.  The chain is the library's one statement of the choice:
 * the direct kernels for a shape without an MFMA plan, else bf16 / split, Winograd, the wave-private 3x3 kernel
 * (opt-in), the weight-stationary 5x5 kernel, the tile instantiation by (MF, KS, CK) and its fused-head variant.
 * name receives the kernel's name as the profiles print it; out = {workgroups, threads per workgroup, dynamic LDS bytes
 * of the launch, MaxDynamicSharedMemorySize the kernel is given once per device (0: none), 1 where the workgroups
 * walk more than one item each}.  A null pointer, a non-positive size, a mode flag that is not one of its values or
 * flags outside DEPGAN_EPF_ALL return status 1; a launch the chosen kernel refuses returns the launcher's status (a
 * fused head on a shape that has none: 1; runs that are no whole chunks, a fused pool on the direct kernels: 3).
 * A refusal writes nothing. */
int depgan_debug_conv_choice(int f32_split, int bf16_mfma, int winograd, int KS, int planN, int B, int H, int W, int Cin,
                             int Cout, unsigned epilogue_flags, int groups, int runs, char* name, int cap, long out[5]);

/* Learning-phase-1 operators (the DEP-UResNet training step's batch-statistics BatchNorm, Dropout, softmax and
 * cross-entropy), each the internal function uresnet.hip calls.  Device pointers; every NHWC view has the float strides
 * (sB, sY, sX) and channel stride 1, so a channel slice of a wider buffer is (p + c0, H*W*Ctot, W*Ctot, Ctot).
 * C % 4 == 0 and (moments, backward) C <= 1024.  scratch_floats: capacity of the reduction scratch the call allocates,
 * <= 0 for what the launch needs; a capacity below that need is refused with status 1, as in the model. */
/* mean[c] and biased var[c] over the B*H*W pixels of x */
int depgan_op_bn_moments(const float* x, long sB, long sY, long sX, int B, int H, int W, int C, float* mean, float* var,
                         long scratch_floats, void* hip_stream);
/* backward of y = gamma*(raw - mean)*rsqrt(var + eps) + beta with batch statistics, for dy*dyscale:
 * dgamma, dbeta (dbeta = sum dy*dyscale) and draw (same strides as dy and raw); invN = 1/(B*H*W) */
int depgan_op_bn_backward(const float* dy, const float* raw, float* draw, long sB, long sY, long sX, int B, int H, int W,
                          int C, const float* gamma, const float* mean, const float* var, float eps, float invN,
                          float dyscale, float* dgamma, float* dbeta, long scratch_floats, void* hip_stream);
/* out = (relu?(film(in*s + t)) dropped) + res; out_pre (optional) = in*s + t; film_mul / film_add (optional): rows of
 * film_ld floats per sample; res (optional); drop_seed 0 = no dropout, else keep when hash >= drop_rate * 2^32 */
int depgan_op_affine_act(const float* in, float* out, float* out_pre, const float* res, long sB, long sY, long sX,
                         const float* s, const float* t, const float* film_mul, const float* film_add, int film_ld,
                         int relu, int B, int H, int W, int C, unsigned drop_seed, float drop_rate, void* hip_stream);
/* softmax over 4 logits per pixel; with onehot: dz = d(mean keras cross-entropy)/dlogits, loss_sum[0] = summed loss.
 * It is depgan_op_softmax_ce with C = 4 and no codes. */
int depgan_op_softmax_ce4(const float* logits, const float* onehot, float* probs, float* dz, float* loss_sum, long P,
                          void* hip_stream);
/* softmax over C = 2..DEPGAN_MAX_HEAD_CLASSES logits per pixel, dense rows (P, C).  Labels: `onehot` (P, C) fp32 or
 * `codes` (P) unsigned char class indices, at most one of them; both NULL: probabilities only (dz, loss_sum unused).
 * With labels dz = d(mean keras cross-entropy)/dlogits and loss_sum[0] = summed loss; the call with codes equals the
 * call with their one-hot encoding bit for bit (the kernel forms t[j] = (j == code) in registers and runs the same
 * statements).  Order of evaluation: the row maximum and the renormalising sum S over the pairs (0,1), (2,3), ...
 * folded left to right, an odd last element last; every other sum over k = 0..C-1 left to right.  A code is only
 * compared, so any byte is safe; pixels with a code >= C add no loss and no gradient, and if there are any the entry
 * returns status 1 with their count (with codes it synchronises the stream for that).  logits, onehot, probs and dz
 * 16-byte aligned where C % 4 == 0, else 4-byte. */
int depgan_op_softmax_ce(const float* logits, const float* onehot, const unsigned char* codes, float* probs, float* dz,
                         float* loss_sum, long P, int C, void* hip_stream);
/* depgan_op_softmax_ce with labels, plus the class census of the same pass: census_host (host, C*C entries, row-major)
 * receives census[tc * C + pc] = the pixels of true class tc predicted as pc.  pc = the first index of the maximum of
 * the probability row as stored in probs (scan k = 0..C-1, replace on a strict >: np.argmax of probs; a tie goes to
 * the lower index).  tc = the code, or with `onehot` the first index of the maximum of the label row (Keras'
 * categorical_accuracy: argmax(y_true); an all-zero row is class 0).  A pixel whose code is >= C is in no bin, so
 * sum(census) + (the count in the message) == P; the entry then returns status 1 as depgan_op_softmax_ce does, with
 * the table written.  probs, dz and loss_sum are bit for bit those of depgan_op_softmax_ce.  The counts are integers
 * summed in two stages without atomics: exact, and independent of what the buffers held before.  Labels are required:
 * a null census_host, or neither onehot nor codes, is status 1 before any HIP call.  Synchronises the stream. */
int depgan_op_softmax_ce_census(const float* logits, const float* onehot, const unsigned char* codes, float* probs,
                                float* dz, float* loss_sum, long long* census_host, long P, int C, void* hip_stream);
/* depgan_op_softmax_ce_census in the loss-weight mode (depgan_uresnet_set_loss_weights states the rule): w_host = n == C
 * host class weights, ignore_code = -1 or a byte value (read with codes only; with onehot the ignored pixel is the
 * all-zero row).  A label pre-pass counts den first; counts_host (host, required) receives its C + 3 counts in the
 * layout of depgan_uresnet_last_label_counts, counts_host[0] = den.  dz carries 1 / den (0 for den = 0) and
 * loss_sum[0] is the weighted sum: the mean is loss_sum / den.  census_host is optional (NULL: no census); under the
 * mode a pixel without a true class joins no bin.  With unit weights and nothing ignored probs, dz and loss_sum are bit
 * for bit those of depgan_op_softmax_ce and den == P.  A negative, NaN or infinite weight, all-zero weights, n != C or
 * an ignore code outside [-1, 255] is status 1 before any HIP call.  A code >= C that is not the ignore code is counted
 * and reported as depgan_op_softmax_ce does (status 1, everything written).  Synchronises the stream. */
int depgan_op_softmax_ce_weighted(const float* logits, const float* onehot, const unsigned char* codes,
                                  const float* w_host, int n, int ignore_code, float* probs, float* dz, float* loss_sum,
                                  long long* census_host, long long* counts_host, long P, int C, void* hip_stream);
/* depgan_op_softmax_ce_weighted in the focal mode (depgan_uresnet_set_focal states the rule): gamma finite and >= 0,
 * label_smoothing in [0, 1); w_host == NULL means unit weights (n is then not read).  A NaN, infinite or negative gamma,
 * a label_smoothing outside [0, 1) and everything depgan_op_softmax_ce_weighted refuses is status 1 before any HIP call,
 * the outputs untouched.  gamma == 0 with label_smoothing == 0 is allowed here and runs the focal statements on the
 * weighted path: den, the counts, the census and probs are those of depgan_op_softmax_ce_weighted, dz and loss_sum agree
 * with it to rounding.  probs are bit for bit those of depgan_op_softmax_ce.  Synchronises the stream. */
int depgan_op_softmax_ce_focal(const float* logits, const float* onehot, const unsigned char* codes, const float* w_host,
                               int n, int ignore_code, float gamma, float label_smoothing, float* probs, float* dz,
                               float* loss_sum, long long* census_host, long long* counts_host, long P, int C,
                               void* hip_stream);
/* The label pre-pass alone, with unit weights: out_host (host, C + 3 entries) in the layout of
 * depgan_uresnet_last_label_counts for P pixels given as onehot (P, C) fp32 or codes (P) unsigned char, exactly one of
 * them.  Integers summed in two stages without atomics.  Synchronises the stream. */
int depgan_op_label_counts(const float* onehot, const unsigned char* codes, long P, int C, int ignore_code,
                           long long* out_host, void* hip_stream);
/* The soft Dice loss at operator level (depgan_uresnet_set_dice_loss states the rule): probs (P, C) fp32 device
 * probabilities as depgan_op_softmax_ce stored them; labels onehot (P, C) fp32 or codes (P) unsigned char, exactly one
 * of them.  ignore_code = -1: every pixel takes part; with codes the pixels of that code stay out (a code >= C always
 * does, and is not counted here); with onehot and ignore_code >= 0 an all-zero row is the pixel that stays out.
 * form, smooth, ce_coef, dice_coef and class_coef_host / n as depgan_uresnet_set_dice_loss takes them.  dz_inout (P, C)
 * device: dz = ce_coef dz + dice_coef dL/dz; with ce_coef == 0 it is written without being read.  sums_host (host,
 * 3 C doubles: I, P, T) and loss_host (host, the Dice term L) are required.  The entry allocates its own scratch and
 * synchronises the stream.  A bad argument is status 1 before any HIP call. */
int depgan_op_dice_loss(const float* probs, const float* onehot, const unsigned char* codes, int ignore_code, int form,
                        const float* class_coef_host, int n, float smooth, float ce_coef, float dice_coef,
                        float* dz_inout, double* sums_host, float* loss_host, long P, int C, void* hip_stream);
/* The signed distance maps of the boundary loss at operator level (depgan_uresnet_set_boundary_loss states the rule):
 * n label slices (H, W) as onehot (n, H, W, C) fp32 or codes (n, H, W) unsigned char, exactly one of them, on the device.
 * ignore_code as depgan_op_dice_loss takes it (-1: every pixel has a true class -- an all-zero one-hot row is class 0,
 * the first arg-max; >= 0: that code, or an all-zero row, has none); a code >= C has none.  class_on_host: NULL (every
 * class), or C host ints, non-zero = the class gets its map; at least one.  phi_out (n, H, W, C) fp32 device: phi of the
 * switched-on classes, 0.0 for the others; every element is written.  sy, sx finite and > 0, inside_offset in
 * [0, min(sy, sx)], H and W in 1..4096, n >= 1, n*H*W < 2^31, C in 2..DEPGAN_MAX_HEAD_CLASSES, phi_out and onehot 4-byte
 * aligned; anything else is status 1 before any HIP call.  Two launches whatever n; the entry allocates its own scratch
 * (2 bytes per pixel and class) and waits for the stream before it frees it.  n*H and the number of 64 x 16 tiles over
 * all slices and classes must each stay below 2^24 (one workgroup each). */
int depgan_op_signed_distance(const float* onehot, const unsigned char* codes, int ignore_code, int n, int H, int W, int C,
                              const int* class_on_host, double sy, double sx, double inside_offset, float* phi_out,
                              void* hip_stream);
/* The boundary loss at operator level: probs (P, C) as depgan_op_softmax_ce stored them, phi (P, C) as
 * depgan_op_signed_distance wrote it, labels and ignore_code as above (they decide m alone).  M = P with
 * ignore_code = -1 (a code >= C then has m = 0 but stays in M: the context refuses such a batch); otherwise
 * M = P - the pixels without a true class - the codes >= C, counted by the label pre-pass on the device.
 * class_coef_host: NULL (1/C each) or ncoef == C host values, finite and >= 0, at least one > 0; boundary_coef finite and
 * >= 0.  dz_inout (P, C) device or NULL: dz += boundary_coef dL_B/dz on the pixels that take part (the others are not
 * written); NULL gives the loss only.  loss_host (host, 2 doubles): L_B and M; M == 0 gives L_B = 0.0 and an untouched
 * dz.  probs, phi, onehot and dz 16-byte aligned where C % 4 == 0, else 4-byte; 1 <= P < 2^31.  Anything else is status 1
 * before any HIP call.  The entry allocates its own scratch and synchronises the stream. */
int depgan_op_boundary_loss(const float* probs, const float* phi, const float* onehot, const unsigned char* codes,
                            int ignore_code, const float* class_coef_host, int ncoef, float boundary_coef,
                            float* dz_inout, double* loss_host, long P, int C, void* hip_stream);
/* The fp32 1x1 head to K = 2..DEPGAN_MAX_HEAD_CLASSES class logits over P pixel rows, as the DEP-UResNet training step
 * runs it for a class count other than 4.  Rows of C floats with a row stride in floats (ld >= C, ld % 4 == 0), so a
 * channel window of a wider buffer is (p + c0, Ctot) with c0 % 4 == 0; C / 4 a power of two <= 64; w (C, K), logits and
 * dz (P, K) dense.  Row bases 16-byte aligned; logits and dz 16-byte aligned where K % 4 == 0, else 4-byte.  Anything
 * else, a null operand, P < 1 or a K outside the range is status 1 before any launch, the outputs untouched.
 * Forward: logits[p][k] = sum_c a[p][c] w[c][k] + b[k].  Order: per 4-channel part a0 w0 then fmaf over channels 1..3,
 * an xor butterfly over the C / 4 parts, + b[k] last. */
int depgan_op_head_k_fwd(const float* a, long ld, const float* w, const float* b, float* logits, long P, int C, int K,
                         void* hip_stream);
/* Backward-data under the ReLU mask of the head's input: din[p][c] = (mask[p][c] > 0) ? sum_k dz[p][k] w[c][k] : +0,
 * the sum as dz0 w0 then fmaf over k = 1..K-1; mask optional (NULL: no mask, ldm unused); mask and din have their own
 * row strides.  Only the C floats of each of the P rows of din are written. */
int depgan_op_head_k_bwd(const float* dz, const float* w, const float* mask, long ldm, float* din, long ldd, long P, int C,
                         int K, void* hip_stream);
/* Weight and bias gradient: dW[c][k] = sum_p a[p][c] dz[p][k] (C, K) dense and db[k] = sum_p dz[p][k], in two stages of
 * fixed order without atomics, so a call repeats bit for bit.  The partials go through a scratch of nb (C K + K) floats,
 * nb <= 1024 the pixel blocks of the launch; the entry allocates it and fills it with NaN first, so the result cannot
 * depend on what it held.  scratch_floats as above: <= 0 for what the launch needs, a capacity below that is status 1.
 * Synchronises the stream. */
int depgan_op_head_k_wgrad(const float* a, long lda, const float* dz, float* dW, float* db, long P, int C, int K,
                           long scratch_floats, void* hip_stream);
/* BatchNorm over the R rows of an [R][ld] matrix (first C columns), moving statistics updated when given:
 * moving = momentum*moving + (1 - momentum)*(mean, var*corr) */
int depgan_op_bn_rows_fwd(const float* x, float* y, int R, int C, int ld, const float* gamma, const float* beta,
                          float eps, float momentum, float corr, float* moving_mean, float* moving_var, float* mean,
                          float* rstd, int relu, void* hip_stream);
/* its backward; relu_out (optional): the forward's ReLU output, dy is masked where it is not positive */
int depgan_op_bn_rows_bwd(const float* dy, const float* x, const float* relu_out, float* dx, int R, int C, int ld,
                          const float* gamma, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                          void* hip_stream);
/* form 0: C[M][N] = A[M][K] B[K][N] (+ bias[N]); 1: C[K][N] = A[M][K]^T B[M][N]; 2: C[M][K] = A[M][N] B[K][N]^T */
int depgan_op_small_gemm(int form, const float* A, const float* Bm, const float* bias, float* Cm, int M, int K, int N,
                         void* hip_stream);

/* The two-critic step's HBM-bound operators and the noise MLP, each the internal function the model calls.  Device
 * pointers; views as above.  scratch_floats: capacity of the reduction scratch the call allocates, <= 0 for what the
 * launch needs; a capacity below that need is refused with status 1. */
/* backward of MaxPooling2D + the ReLU mask of its input a (pooled Ho x Wo, full 2Ho x 2Wo):
 * out = ((first arg-max of the 2x2 window of a) ? dpool : 0) + skip) * (a > 0); skip optional (NULL). C % 4 == 0 */
int depgan_op_unpool_mask(const float* dpool, long dsB, long dsY, long dsX, const float* a, long asB, long asY, long asX,
                          const float* skip, long ssB, long ssY, long ssX, float* out, long osB, long osY, long osX,
                          int B, int Ho, int Wo, int C, void* hip_stream);
/* out[pooled] = u[first arg-max of the 2x2 window of a] */
int depgan_op_gather_pool(const float* u, long usB, long usY, long usX, const float* a, long asB, long asY, long asX,
                          float* out, long osB, long osY, long osX, int B, int Ho, int Wo, int C, void* hip_stream);
/* generator head over [P][C] rows.  backward 0: out[p] = act(a[p] . w + b[0]), act tanh or identity;
 * backward 1: out[p][c] = dpre[p] * w[c] * (a[p][c] > 0).  C/4 a power of two <= 64 */
int depgan_op_head(int backward, const float* a, const float* w, const float* b, const float* dpre, float* out, long P,
                   int C, int tanh_act, void* hip_stream);
/* critic tail over N samples of [HW][C]: t9[n][p] = a . w9 + b9 ; out[n] = sum_p wd[p] t9[n][p] + bd */
int depgan_op_critic_tail_fwd(const float* a, const float* w9, const float* b9, const float* wd, const float* bd,
                              float* t9, float* out, int N, int HW, int C, void* hip_stream);
/* dz[n][p][c] = coefs[n / per] * wd[p] * w9[c] * (a[n][p][c] > 0) */
int depgan_op_critic_tail_bwd(const float* a, const float* w9, const float* wd, const float* coefs, int per, float* dz,
                              int N, int HW, int C, void* hip_stream);
/* the tail's weight gradients from coefs[n / per] * src; accumulate 1 adds to dw9 / dwd (/ db9 / dbd) */
int depgan_op_critic_tail_wgrad(const float* src, const float* w9, const float* b9, const float* wd, const float* coefs,
                                int per, int add_bias_terms, int accumulate, float* dw9, float* db9, float* dwd,
                                float* dbd, int N, int HW, int C, long scratch_floats, void* hip_stream);
/* column sums of an NHWC view: out[c] (+)= scale[c] (or 1) * sum, raw[c] = sum (out, raw optional); with rowmul:
 * out[c] = sum_q rowmul[q] v[q][c] over the dense pixel index q (then scale, raw, accumulate must be unset).
 * C % 4 == 0, C <= 256 */
int depgan_op_colsum(const float* v, long sB, long sY, long sX, int B, int H, int W, int C, const float* scale,
                     float* out, float* raw, int accumulate, const float* rowmul, long scratch_floats, void* hip_stream);
/* out[0] = sum in[0..n) */
int depgan_op_sum(const float* in, long n, float* out, long scratch_floats, void* hip_stream);
/* which 0 / 1: the [real | fake | ep-mixed] input batch of the Y2 / DEM critic (3*B*HW floats);
 * which 2: out = x[..., 0] + attr (B*HW floats; y2 and ep unused).  x has nicg interleaved channels */
int depgan_op_critic_inputs(const float* y2, const float* x, int nicg, const float* attr, const float* ep, float* out,
                            int B, long HW, int which, void* hip_stream);
/* norms[b] = ||g0[b]||, u0 = delta*(2/B)*(norm-1)/norm * g0, gp_out (optional) = mean (norm-1)^2 */
int depgan_op_gp_u0(const float* g0, float* u0, float* norms, float* gp_out, float delta, int B, long HW,
                    long scratch_floats, void* hip_stream);
/* out = [sum d_out[0..B), sum d_out[B..2B), sum (norms-1)^2, B] */
int depgan_op_critic_stats(const float* d_out, const float* norms, float* out, int B, void* hip_stream);
/* sums = [sum |attr-(y2-y1)|, #(y2 >= thr), #(y1+attr >= thr), #(both)], y1 = x[..., 0] */
int depgan_op_gloss_sums(const float* x, int nicg, const float* y2, const float* attr, float thr, float* sums, long P,
                         long scratch_floats, void* hip_stream);
/* dpre = (-(g1+g2)/B + (100/P) sign(attr - (y2-y1))) * (1 - attr^2) */
int depgan_op_g_dpre(const float* x, int nicg, const float* y2, const float* attr, const float* g1, const float* g2,
                     float* dpre, int B, long P, void* hip_stream);
/* FiLM backward over [B][HW][C]; fmul/fadd and dmul/dadd are rows of film_ld floats per sample.  C % 4 == 0, C <= 128 */
int depgan_op_film_bwd(const float* dr, const float* u, const float* fmul, const float* fadd, int film_ld, float* du,
                       float* dmul, float* dadd, int B, long HW, int C, long scratch_floats, void* hip_stream);
/* one launch over njobs BatchNorm affines; ptrs: 8 device pointers per job (gamma, beta, mean, var, s, t, rstd,
 * mean_copy or NULL), C: channels per job (host arrays) */
int depgan_op_bn_prepare_batch(void* const* ptrs, const int* C, int njobs, float eps, void* hip_stream);
/* one launch over njobs BN-gamma gradients; ptrs: 7 device pointers per job (W, dWraw, bias, mean, rstd, S, dgamma),
 * dims: K, Cout, oi, Cin per job (host arrays); the jobs' blocks follow each other, Cout per job */
int depgan_op_bn_gamma_grad_batch(void* const* ptrs, const int* dims, int njobs, void* hip_stream);
/* the noise MLP with inference-mode BatchNorm.  trunk: W0, b0, s0, t0, mean0, rstd0 (32 each), W1 (32x32), b1, s1, t1,
 * mean1, rstd1 (32 each); Wh: the 14 head kernels [1024][ncol[h]] back to back; hvec: bh, sh, th, meanh, rstdh
 * (1024 each); ncol: 14 host ints summing to 1024; acts: h0, a0, h1, a1, lin, heads ([B][1024] each) */
int depgan_op_noise_fwd(const float* trunk, const float* Wh, const float* hvec, const int* ncol, const float* z,
                        float* acts, int B, void* hip_stream);
/* its backward from dheads [B][1024]: gtrunk = dW0, db0, dgamma0, dbeta0 (32 each), dW1 (32x32), db1, dgamma1, dbeta1;
 * dWh packed as Wh; ghvec = dbh, dgamma_h, dbeta_h (1024 each) */
int depgan_op_noise_bwd(const float* trunk, const float* Wh, const float* hvec, const int* ncol, const float* z,
                        float* acts, const float* dheads, float* gtrunk, float* dWh, float* ghvec, int B,
                        long scratch_floats, void* hip_stream);
/* best-of-k noise: k x 8 loss pieces -> *best = np.argmin of the k total losses, z_out = z_all[best] (zfloats) */
int depgan_op_best_noise(const float* stats, int k, const float* z_all, long zfloats, int* best, float* z_out,
                         void* hip_stream);
/* dst[i] = mask[i] ? float(bfloat16(src[i])) : src[i] */
int depgan_op_round_bf16_masked(const float* src, const unsigned char* mask, float* dst, long n, void* hip_stream);
/* The kernels behind depgan_set_optimizer on caller-owned device arrays; both allocate their scratch and synchronise.
 * depgan_op_grad_sqnorm: *out_host = sum_i ((double)(g[i] * gscale))^2 (g 16-byte aligned), bit-identical from run to run.
 * depgan_op_adam_opts: one update of p, m, v (n floats each) by the option kernel, whatever the options (all 0 runs it with
 *   nothing acting, which gives the plain kernel's bits).  lr_t is the bias-corrected rate, lr the plain one (it only
 *   scales weight_decay).  seg_end_host (nseg ascending element ends, the last one n) and seg_decay_host (nseg flags)
 *   say which elements weight_decay acts on; nseg = 0: none.  With clipnorm > 0 the squared norm is taken from g first
 *   and norm_host[0] = the norm, norm_host[1] = the scale used (0: the norm was not finite and nothing was written);
 *   otherwise norm_host (optional) gets 0 and 1. */
int depgan_op_grad_sqnorm(const float* g, long n, float gscale, double* out_host, void* hip_stream);
int depgan_op_adam_opts(float* p, const float* g, float* m, float* v, long n, float lr_t, float lr, float b1, float b2,
                        float eps, float gscale, float clipnorm, float clipvalue, float weight_decay,
                        const long* seg_end_host, const int* seg_decay_host, int nseg, double* norm_host,
                        void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
