/*
 * mmf_hip.h — C-ABI of libmmf_hip.so, the MI355X-native (gfx950) hot path of the reference's
 * MisinfoForensics.analyze() 5-signal forward.
 *
 * The reference has no FFI: its boundary is the Python API of misinfo_forensics.py.  Each entry
 * point below replaces one reference call site; the Python host side (mmf_amd/hip.py, ctypes)
 * keeps the reference's method names and return dicts on top of these.
 *
 * Conventions
 *   - Plain C types only; every function returns 0 on success or a negative errno-style code
 *     (MMF_EINVAL bad argument/shape/missing weight, MMF_ENOMEM allocation, MMF_EIO HIP error).
 *     Nothing throws across the ABI.  mmf_last_error() gives a thread-local message.
 *   - All tensor I/O of the forward calls are caller-owned DEVICE pointers (e.g. torch tensors'
 *     data_ptr()), enqueued asynchronously on the caller's hipStream_t `stream` (NULL = default
 *     stream).  No implicit device synchronisation.
 *   - Weights, workspaces and the Truth-Vault are owned by the handle.  A handle is bound to one
 *     device and is not thread-safe: one handle per (process, device).
 *   - Layouts: token ids / masks int32 row-major [B, L]; images uint8 [B, 224, 224, 3] (HWC, RGB);
 *     embeddings / logits / scores fp32 row-major.
 */
#ifndef MMF_HIP_H
#define MMF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMF_OK 0
#define MMF_EINVAL (-22)
#define MMF_ENOMEM (-12)
#define MMF_EIO (-5)
#define MMF_ERANGE (-34) /* an input outside a kernel's supported range (mmf_resize_pil: too many taps) */
#define MMF_EUNSUPPORTED (-95) /* a valid input of a kind this path does not handle (mmf_jpeg_*: CMYK, lossless, coefficients outside the exact range, ...) */

#define MMF_DTYPE_F32 0
#define MMF_DTYPE_I64 1

typedef struct mmf_handle mmf_handle;

/* Create a handle on HIP device `device` (ordinal within HIP_VISIBLE_DEVICES). */
int mmf_create(int device, mmf_handle** out);
void mmf_destroy(mmf_handle* h);
/* Thread-local description of the last error (empty string if none). */
const char* mmf_last_error(void);
/* Library/ABI version string. */
const char* mmf_version(void);

/* Stage one host tensor under its state-dict name.  Names are the reference's state-dict keys:
 * detector keys as in MultiModalMisinfoDetector (misinfo_forensics.py:43-108 — "roberta.*",
 * "ai_head.*", "misinfo_head.*", "efficientnet.*", "fusion_layer.*") and CLIP keys as in HF
 * CLIPModel prefixed with "clip." (misinfo_forensics.py:210-212).  Replaces the reference's
 * load_state_dict (misinfo_forensics.py:175-186, 260-317); the data are copied. */
int mmf_load_tensor(mmf_handle* h, const char* name, int dtype, int ndim, const int64_t* shape,
                    const void* host_data);
/* Pack staged tensors into device layouts (fused QKV, BatchNorm folded into convs, fp16 GEMM
 * operands).  Components whose tensors are all present become available; `clip_eos_token_id`
 * selects the HF EOS-pooling rule (2 = argmax(ids), else first index of that id;
 * TF clip:561-582). */
int mmf_finalize(mmf_handle* h, int clip_eos_token_id);
/* Bit mask of ready components: 1 text(RoBERTa+heads) 2 effnet 4 clip-vision 8 clip-text
 * 16 fusion 32 vault. */
int mmf_ready(mmf_handle* h);

/* Allocate activation workspaces for up to `max_batch` rows with RoBERTa length `max_text_len`
 * (<= 512) and CLIP text length `max_clip_len` (<= 77).  Forward calls with larger shapes fail
 * with MMF_EINVAL; call before graph capture. */
int mmf_reserve(mmf_handle* h, int max_batch, int max_text_len, int max_clip_len);

/* Signals 1-2 — analyze_text (misinfo_forensics.py:319-352): RoBERTa + dual heads.
 * ids/mask int32 [B, L <= 512] device (the reference tokenizer truncates at 512, :327-333; L > 128
 * takes the long-sequence attention kernel).  Outputs fp32 [B, 2] logits each (may be NULL) and
 * scores fp32 [B, 2] = softmax(.)[:,1] of (ai, misinfo) (may be NULL). */
int mmf_text_forward(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L,
                     float* ai_logits, float* misinfo_logits, float* scores2, void* stream);

/* The frozen part of the text-head training script (train_ai_head.py:415-420 freezes everything but the
 * head, :224-230 runs the whole encoder for every minibatch of every epoch): the rows the two heads read,
 * outputs.last_hidden_state[:, 0, :] (misinfo_forensics.py:95).  ids/mask as mmf_text_forward; cls fp32
 * [B, 768], 16-byte aligned.  The launch sequence of mmf_text_forward in the stream layout in use
 * (fp16, split or precise), without the heads; a sequence whose fp16 stream overflowed gets a NaN row, as
 * it gets NaN logits there. */
int mmf_text_pooled(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* cls, void* stream);

/* Training of one RoBERTa text head -- ai_head or misinfo_head, Linear(768,256)-ReLU-Dropout-Linear(256,2)
 * (misinfo_forensics.py:57-69) -- on cached CLS rows (train_ai_head.py:206-255 the loop body of train_epoch,
 * stated for the deployed head): ONE epoch.  For each of the ceil(N / batch) minibatches: pre = X W1^T +
 * b1; h = relu(pre) * keep * scale, scale = fp32 of 1 / (1 - p_drop) computed in double; logits = h W2^T +
 * b2; mean cross-entropy; backward to all four tensors; clip_grad_norm_ over them together (coefficient
 * max_norm / (norm + 1e-6), clamped at 1, always applied); torch.optim.AdamW (decoupled decay on all four,
 * bias correction by step0 + s + 1) with the learning rate lr_steps[s] of that step (the script steps its
 * warmup-cosine schedule after every minibatch, :241; a step with lr 0 leaves the parameters bit-unchanged
 * and still updates the moments).  No handle; asynchronous on `stream` as a chain of four ordinary
 * launches per minibatch (no grid barrier, no atomics).  All fp32; every reduction has a fixed order
 * (csrc/head_train.hip), so results are bit-reproducible and do not depend on how an epoch is split into
 * launches.
 *   feat fp32 [N][768]; labels int32 [N], read as label & 1; perm int32 [N]: minibatch s takes positions
 *     s*batch .. of perm (the last may be short; its mean is over its own rows); an entry outside [0, N)
 *     is clamped, so no input makes a kernel read out of bounds.
 *   keep uint64 [N][4] or NULL: keep[i] is the dropout mask of the row at POSITION i of the epoch order,
 *     word w bit j set = hidden unit 64 w + j kept and scaled; NULL = no dropout, no scaling.
 *   lr_steps: HOST double [nsteps], read before the call returns.
 *   params, exp_avg, exp_avg_sq fp32 [MMF_HEAD_PARAMS], state-dict order, updated in place.
 *   step_loss fp32 [nsteps]: the minibatch's mean loss (train-mode logits, before its update); step_correct
 *     int32 [nsteps]: rows with argmax(logits) == label (a tie is class 0, as torch.argmax); step_gnorm fp32
 *     [nsteps]: the unclipped total norm; grad_out fp32 [MMF_HEAD_PARAMS] or NULL: the last minibatch's
 *     clipped gradient.
 *   ws: ws_bytes >= what the sizing call returns for `batch` (0 for a batch outside 1..64).
 * feat, params, the moments, grad_out and ws are 16-byte aligned, keep 8-byte.  MMF_EINVAL with nothing
 * launched: a NULL required pointer, N < 1, batch outside 1..64, p_drop outside [0, 1), a short or
 * misaligned ws. */
#define MMF_HEAD_PARAMS 197378  /* 0.weight[256][768], 0.bias[256], 3.weight[2][256], 3.bias[2] */
int64_t mmf_head_train_ws_bytes(int batch);
int mmf_head_train_epoch(const float* feat, const int32_t* labels, int N, const int32_t* perm, const uint64_t* keep,
                         float p_drop, int batch, const double* lr_steps, double beta1, double beta2, double eps,
                         double weight_decay, double max_norm, int step0, float* params, float* exp_avg,
                         float* exp_avg_sq, float* step_loss, int32_t* step_correct, float* step_gnorm, float* grad_out,
                         void* ws, int64_t ws_bytes, void* stream);

/* validate (train_ai_head.py:258-296) on cached CLS rows: forward only, no dropout, consecutive batches in
 * file order.  batch_loss fp32 [ceil(N / batch)]: each batch's mean cross-entropy; row_logits fp32 [N][2].
 * ws and the errors as the training call's. */
int mmf_head_eval(const float* feat, const int32_t* labels, int N, int batch, const float* params, float* batch_loss,
                  float* row_logits, void* ws, int64_t ws_bytes, void* stream);

/* Signal 3 — analyze_image (misinfo_forensics.py:354-373, 249-253): ImageNet normalisation +
 * EfficientNet-B0.  img uint8 [B, 224, 224, 3] device.  logits fp32 [B, 2] (may be NULL),
 * deepfake_score fp32 [B] (may be NULL). */
int mmf_effnet_forward(mmf_handle* h, const uint8_t* img, int B, float* logits, float* deepfake_score,
                       void* stream);

/* Same as mmf_effnet_forward for an already-normalised fp32 NCHW tensor x [B, 3, 224, 224] (the
 * reference's detector.forward_image(image_tensor) signature, misinfo_forensics.py:102-104). */
int mmf_effnet_forward_f32(mmf_handle* h, const float* x, int B, float* logits, float* deepfake_score,
                           void* stream);

/* The frozen part of the deepfake-classifier training (train_cifake_forensics.py runs the whole backbone for
 * every minibatch of every epoch): the row the deployed classifier reads, the global average over the 7x7
 * head output (misinfo_forensics.py:72-76).  img as mmf_effnet_forward; pooled fp32 [B, 1280], 16-byte
 * aligned.  The launch sequence of mmf_effnet_forward for the tower in use (fp16, or fp32 under option
 * effnet_fp32) on one stream, without the classifier: per channel the pixels summed in ascending order in
 * fp32, times 1 / 49, as the classifier kernels form it.  An overflowed fp16 activation gives a non-finite
 * row, as it gives a non-finite score there. */
int mmf_effnet_pooled(mmf_handle* h, const uint8_t* img, int B, float* pooled, void* stream);

/* The frozen part of the head-stage training (mmf_effhead_train_epoch below): the output of the last MBConv
 * block, what the head conv features.8 reads.  img as mmf_effnet_pooled; trunk fp32 [B, 49, 320], 16-byte
 * aligned: positions row-major over 7 x 7, channels innermost.  The launch sequence of the tower in use
 * without the head GEMM, the pool and the classifier; the fp16 tower's values are converted to fp32 exactly,
 * the fp32 tower's are copied.  Errors as mmf_effnet_pooled's. */
int mmf_effnet_trunk(mmf_handle* h, const uint8_t* img, int B, float* trunk, void* stream);

/* RandomHorizontalFlip's mirror on a staged uint8 window (train_cifake_forensics.py:39-45: Resize, then the
 * flip): dst[b][y][x][c] = src[b][y][W-1-x][c].  No handle.  dst and src must not overlap.  MMF_EINVAL with
 * nothing launched: a NULL pointer, a non-positive dimension, dst == src. */
int mmf_hflip_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, void* stream);

/* ColorJitter on staged uint8 windows (train_cifake_forensics.py:39-45: Resize, the flip, then
 * ColorJitter(0.2, 0.2, 0.2, 0.1), all before ToTensor), byte-exact with what torchvision's PIL backend computes
 * with Pillow: ImageEnhance.Brightness / Contrast / Color (Image.blend against black / the rounded mean of L / L)
 * and, for the hue, convert("HSV"), a uint8 wrap-around add on H and convert("RGB").  src, dst uint8 [B][H][W][3],
 * any H, W >= 1; dst and src must not overlap.  No handle; two ordinary launches on `stream`, no atomics: the
 * first forms, for images whose chain holds a contrast, the sum of L of the image as it stands at that point of
 * the chain (integer partial sums per chunk of pixels in ws, so the result does not depend on any order), the
 * second applies the chain.
 *   ops int32 [B][4]: the k-th operation applied to image b: 0 brightness, 1 contrast, 2 saturation, 3 hue,
 *     -1 skip.  The result of every operation is rounded to uint8 before the next, as in the PIL chain.  A chain
 *     holds at most one contrast: a second one is skipped, as is any code outside -1..3.
 *   factors fp32 [B][3]: brightness, contrast, saturation (the blend factor: 1 keeps the image; 0 <= f <= 1
 *     truncates, any other factor clips, as Image.blend does).
 *   hue_shift int32 [B]: what is added to H, taken & 255 (torchvision: uint8(hue_factor * 255)).  A hue operation
 *     with shift 0 still makes the HSV round trip, which is not the identity.
 *   ws uint64 [B][MMF_JITTER_CHUNKS], 8-byte aligned; contents on entry do not matter.
 * No value in the device arrays can make a kernel read or write out of bounds.  MMF_EINVAL with nothing launched
 * and dst untouched: a NULL pointer, a non-positive dimension, B > 65535 (the grid), H * W > 2^40 (the sum of L
 * must stay exact in a double), dst == src, ops / factors / hue_shift not 4-byte aligned, ws not 8-byte. */
#define MMF_JITTER_CHUNKS 256
int mmf_color_jitter_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* ops, const float* factors,
                        const int32_t* hue_shift, uint64_t* ws, void* stream);

/* GaussianBlur on staged uint8 windows (misinformation_dataset.py:104-125: RandomApply([GaussianBlur(kernel_size=
 * (5, 9), sigma=(0.1, 5.0))], p=0.3) between ColorJitter and RandomJPEGCompression), as torchvision's tensor
 * backend computes it for a PIL image: float32 sums over a KY x KX window (KX the width) with reflected borders,
 * the edge sample not repeated, rounded half to even.  src, dst uint8 [B][H][W][3]; dst and src must not overlap.
 * No handle, no workspace; one ordinary launch on `stream`, no atomics.
 *   weights fp32 [B][KY][KX]: image b's window, formed on the host (torch's own floats: the device evaluates no
 *     exp).
 *   apply int32 [B]: 0 copies image b unchanged (a RandomApply that did not fire), anything else blurs it.
 * The order of the float32 operations is fixed: per output byte acc = 0, then for i = 0 .. KY - 1 (outer) and
 * j = 0 .. KX - 1 (inner) acc = acc + w[i][j] * byte(y + i - KY/2, x + j - KX/2) with the product rounded before
 * the add (no FMA), then rintf, a clamp to 0..255 (a NaN gives 0) and the byte.  torch's conv2d adds in another
 * order, so a byte may differ from it by one where the exact sum is within float32 rounding of a half.
 * (KX, KY) = (5, 9) has a kernel of its own; every other odd pair up to 15 runs with run-time tap counts, same
 * arithmetic.  No value in the device arrays can make the kernel read or write out of bounds.  MMF_EINVAL with
 * nothing launched and dst untouched: a NULL pointer, B outside 1..65535 (the grid), H or W < 1, H * W > 2^30
 * (tile and byte indices), KX or KY even or outside 1..15, W <= KX/2 or H <= KY/2 (where torch's reflection pad
 * raises), dst overlapping src anywhere (the byte ranges are compared), weights or apply not 4-byte aligned. */
int mmf_gaussian_blur_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int KX, int KY, const float* weights,
                         const int32_t* apply, void* stream);

/* RandomJPEGCompression on staged uint8 windows (misinformation_dataset.py:18-57: the image saved as a JPEG at a
 * random quality and loaded back), byte-exact with Pillow's Image.save(format="JPEG", quality=q, optimize=False)
 * followed by Image.open(...).convert("RGB").  Huffman coding is lossless, so no bit stream is formed: libjpeg's
 * forward half (RGB -> YCbCr, 4:2:0 downsampling with the edges replicated, the islow forward DCT, quantisation by
 * jpeg_set_quality's tables) runs straight into the inverse half of the device decoder below (dequantisation, the
 * islow IDCT, fancy upsampling, YCbCr -> RGB).  src, dst uint8 [B][H][W][3], any H, W >= 1; dst and src must not
 * overlap.  No handle, no atomics; on `stream`: flags cleared, then two ordinary launches (per 8x8 block of a
 * component everything up to the range-limited samples, in registers, into ws; per pixel the upsampling and the
 * colour conversion).
 *   quality int32 [B]: 1..100, or 0: image b is copied unchanged.  Any other value is treated as 0.
 *   ws: mmf_jpeg_roundtrip_ws_bytes(H, W) bytes per image (host-only; 0 for a shape the call rejects), 8-byte
 *     aligned: the sample planes; contents on entry do not matter.
 *   flags int32 [B], written by the call: 0, or 1 where a block of image b left the exact range of the decoder
 *     (see "The exact range" below; the three conditions are evaluated on the block's own values).  dst[b] is then
 *     not Pillow's bytes and the caller redoes that image on the host.  No block made from pixels has been seen to
 *     leave the range.
 * No value in the device arrays can make a kernel read or write out of bounds.  MMF_EINVAL with nothing launched
 * and dst untouched: a NULL pointer, a non-positive dimension, B > 65535 (the grid), H * W > 2^30 (pixel indices
 * are ints), dst == src, quality / flags not 4-byte aligned, ws not 8-byte. */
int64_t mmf_jpeg_roundtrip_ws_bytes(int H, int W);
int mmf_jpeg_roundtrip_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* quality, uint8_t* ws,
                          int32_t* flags, void* stream);

/* Training of the deployed deepfake classifier -- Dropout(0.2) then Linear(1280, 2) on the pooled row
 * (misinfo_forensics.py:72-76) -- on cached pooled rows (train_cifake_forensics.py:187-216 the loop body, stated
 * for a frozen backbone): ONE epoch in ONE launch by one workgroup.  For each of the ceil(N / batch)
 * minibatches: xd = x * keep * scale, scale = fp32 of 1 / (1 - p_drop) computed in double; logits = xd W^T + b;
 * mean cross-entropy; backward to both tensors; torch.optim.Adam (:334-337): weight_decay * p added to the
 * gradient (0 leaves it bit-unchanged), bias correction by step0 + s + 1, constant lr, no clipping.  No
 * handle; asynchronous on `stream`.  All fp32, the step scalars computed in double from the step number
 * alone; every reduction has a fixed order that depends on the minibatch's row count alone
 * (csrc/effnet_train.hip), so results are bit-reproducible and do not depend on how an epoch is split into
 * launches.
 *   feat fp32 [R][1280], labels int32 [R] (read as label & 1): a BANK of R rows; perm int32 [N]: the epoch's
 *     N entries, each a bank row (an entry outside [0, R) is clamped, so no input makes the kernel read out
 *     of bounds).  Minibatch s takes positions s*batch .. of perm; the last may be short (its mean is over
 *     its own rows).  R and N are separate so that a caller can offer a second view of every image (the
 *     mirrored one) as further bank rows.
 *   keep uint64 [N][20] or NULL: keep[i] is the dropout mask of the row at POSITION i of the epoch order,
 *     word w bit j set = input channel 64 w + j kept and scaled; NULL = no dropout, no scaling.
 *   params, exp_avg, exp_avg_sq fp32 [MMF_EFFCLS_PARAMS], state-dict order, updated in place.
 *   step_loss fp32 [nsteps]: the minibatch's mean loss (train-mode logits, before its update); step_correct
 *     int32 [nsteps]: rows with argmax(logits) == label (a tie is class 0, as torch.max); grad_out fp32
 *     [MMF_EFFCLS_PARAMS] or NULL: the last minibatch's loss gradient (what p.grad holds: without the decay).
 * Buffers are 4-byte aligned, keep 8-byte.  MMF_EINVAL with nothing launched: a NULL required pointer, R < 1,
 * N < 1, batch outside 1..64, step0 < 0, p_drop outside [0, 1), a misaligned buffer. */
#define MMF_EFFCLS_PARAMS 2562  /* classifier.1.weight [2][1280], classifier.1.bias [2] */
int mmf_effcls_train_epoch(const float* feat, const int32_t* labels, int R, const int32_t* perm, int N,
                           const uint64_t* keep, float p_drop, int batch, double lr, double beta1, double beta2,
                           double eps, double weight_decay, int step0, float* params, float* exp_avg,
                           float* exp_avg_sq, float* step_loss, int32_t* step_correct, float* grad_out, void* stream);

/* validate (train_cifake_forensics.py:236-276) on cached pooled rows: forward only, no dropout, consecutive
 * batches of the R bank rows in file order, one workgroup per batch.  batch_loss fp32 [ceil(R / batch)]: each
 * batch's mean cross-entropy; row_logits fp32 [R][2].  Errors as the training call's. */
int mmf_effcls_eval(const float* feat, const int32_t* labels, int R, int batch, const float* params,
                    float* batch_loss, float* row_logits, void* stream);

/* Training of EfficientNet's head conv stage -- features.8 = Conv2d(320, 1280, 1, bias=False) + BatchNorm2d(1280)
 * + SiLU -- jointly with the classifier above, on cached trunk rows (mmf_effnet_trunk).  The BatchNorm runs in
 * EVAL mode: its running statistics bn_mean / bn_var fp32 [1280] and bn_eps are inputs and never written, so a
 * row does not depend on its minibatch (the script trains in model.train()).  Per minibatch of
 * n <= 64 images, M = 49 n rows:
 *   z = x W^T; s_c = gamma_c / sqrt(var_c + eps), t_c = beta_c - mean_c s_c; y = s_c z + t_c; a = y / (1 + exp(-y));
 *   pooled[r][c] = (sum over the 49 positions, ascending) / 49; from here mmf_effcls_train_epoch's contract:
 *   xd = pooled * keep * scale, logits, mean cross-entropy, torch.optim.Adam on ALL parameters (L2 decay added
 *   to the gradient, bias correction by step0 + s + 1, constant lr).  Backward: dpooled = keep scale dl Wc,
 *   dy = dpooled / 49 * sig (1 + y (1 - sig)), dgamma_c = sum dy (z - mean_c) / sqrt(var_c + eps), dbeta_c =
 *   sum dy, dW[c][k] = sum (dy s_c) x[.][k]; no gradient with respect to the trunk.
 * params, exp_avg, exp_avg_sq fp32 [MMF_EFFHEAD_PARAMS], state-dict order: features.8.0.weight [1280][320] |
 * features.8.1.weight [1280] | features.8.1.bias [1280] | classifier.1.weight [2][1280] | classifier.1.bias [2].
 * trunk fp32 [R][49][320]; labels, perm, keep, step_loss, step_correct, grad_out as mmf_effcls_train_epoch's (a
 * perm entry outside [0, R) is clamped; keep is the mask on the POOLED row).  ws: mmf_effhead_ws_bytes(batch) bytes
 * (host arithmetic; 0 for a batch outside 1..64), contents on entry do not matter.  No handle; three ordinary
 * launches per minibatch on `stream`, no host synchronisation, no atomics.  All fp32; both contractions on the
 * fp32-input MFMA, each output one fmaf chain in ascending order; every reduction has one fixed order
 * (csrc/effhead_train.hip), so results are bit-reproducible and do not depend on how an epoch is split into calls.
 * trunk, params, exp_avg, exp_avg_sq, grad_out and ws are 16-byte aligned, keep 8-byte, the rest 4-byte.
 * MMF_EINVAL with nothing launched: what mmf_effcls_train_epoch rejects, a ws that is too small or misaligned, a
 * bn_eps that is not finite and positive as the fp32 value the kernels use. */
#define MMF_EFFHEAD_PARAMS 414722
int64_t mmf_effhead_ws_bytes(int batch);
int mmf_effhead_train_epoch(const float* trunk, const int32_t* labels, int R, const int32_t* perm, int N,
                            const uint64_t* keep, float p_drop, int batch, const float* bn_mean, const float* bn_var,
                            double bn_eps, double lr, double beta1, double beta2, double eps, double weight_decay,
                            int step0, float* params, float* exp_avg, float* exp_avg_sq, float* step_loss,
                            int32_t* step_correct, float* grad_out, void* ws, int64_t ws_bytes, void* stream);

/* validate on cached trunk rows: forward only, no dropout, consecutive batches of the R bank rows in file order,
 * two launches per batch.  batch_loss fp32 [ceil(R / batch)], row_logits fp32 [R][2]; a row's logits do not depend
 * on the batch size.  Errors as the training call's. */
int mmf_effhead_eval(const float* trunk, const int32_t* labels, int R, int batch, const float* params,
                     const float* bn_mean, const float* bn_var, double bn_eps, float* batch_loss, float* row_logits,
                     void* ws, int64_t ws_bytes, void* stream);

/* CLIP image embedding — get_image_features + L2 normalisation (misinfo_forensics.py:395-401,
 * 432-439).  img uint8 [B, 224, 224, 3] (CLIP-preprocessed geometry); emb fp32 [B, 512] unit. */
int mmf_clip_image(mmf_handle* h, const uint8_t* img, int B, float* emb_unit, void* stream);

/* CLIP text embedding — get_text_features + L2 normalisation (misinfo_forensics.py:395-401,
 * 473-481).  ids/mask int32 [B, L<=77]; emb fp32 [B, 512] unit. */
int mmf_clip_text(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* emb_unit,
                  void* stream);

/* analyze_consistency (misinfo_forensics.py:375-408) / CLIPSimilarityEngine.calculate_similarity
 * (clip_similarity_engine.py:63-119): both CLIP towers (text tower on a concurrent stream) and the
 * cosine of the unit embeddings.  img uint8 [B,224,224,3], ids/mask int32 [B, L<=77]; sim fp32 [B];
 * img_emb / txt_emb fp32 [B, 512] unit (may be NULL: handle workspaces are used). */
int mmf_clip_consistency(mmf_handle* h, const uint8_t* img, const int32_t* ids, const int32_t* mask, int B, int L,
                         float* img_emb, float* txt_emb, float* sim, void* stream);

/* The frozen part of CLIPDetective (train_clip_detective.py:89-99, 119-122: what every minibatch of
 * every epoch recomputes there): the pooled rows the projection heads read.  Inputs as those of the
 * consistency call above; img_pooled fp32 [B, 768] = post_layernorm of the CLS row, txt_pooled fp32
 * [B, 512] = final_layer_norm of the EOS row.  Either output may be NULL: that tower is not run (its
 * inputs may then be NULL too).  Same towers, streams and stream precision as the embedding calls. */
int mmf_clip_pooled(mmf_handle* h, const uint8_t* img, const int32_t* ids, const int32_t* mask, int B, int L,
                    float* img_pooled, float* txt_pooled, void* stream);

/* Trained projection heads back into a handle (the load_state_dict of train_clip_detective.py:498-500
 * for the two trained matrices): device fp32 visual [512][768] / text [512][512], rounded to fp16
 * into the buffers the towers read.  Either may be NULL.  Allocates nothing. */
int mmf_set_clip_projections(mmf_handle* h, const float* visual_f32, const float* text_f32, void* stream);

/* CLIPDetective training on cached pooled features (train_clip_detective.py:129-166 the loss,
 * :203-225 the loop body of train_epoch): ONE epoch.  For each of the ceil(N / batch) minibatches:
 * e = P W^T per tower, divided by its row norm (no epsilon); logits = exp(logit_scale) I T^T; the mean
 * of the two cross-entropies against the diagonal; backward to all three parameters; clip_grad_norm_
 * over them together (coefficient max_norm / (norm + 1e-6), clamped at 1, always applied);
 * torch.optim.AdamW (decoupled decay on all three, bias correction by step0 + s + 1).  No handle;
 * asynchronous on `stream` as a chain of ordinary launches (no grid barrier, no atomics).  All fp32;
 * every reduction has a fixed order, so results are bit-reproducible and do not depend on how an
 * epoch is split into launches.
 *   img_feat fp32 [N][768], txt_feat fp32 [N][512]; perm int32 [N]: minibatch s takes positions
 *     s*batch .. of perm (the last may be short); an entry outside [0, N) is clamped.
 *   params, exp_avg, exp_avg_sq fp32 [MMF_CLIP_TRAIN_PARAMS], updated in place.
 *   step_loss fp32 [nsteps]: the minibatch loss before its update; step_gnorm fp32 [nsteps]: the
 *     unclipped total norm; grad_out fp32 [MMF_CLIP_TRAIN_PARAMS] or NULL: the last minibatch's
 *     clipped gradient.
 *   ws: ws_bytes >= what the sizing call returns for `batch` (0 for a batch outside 1..64).
 * Pointers are 16-byte aligned.  A 1-row minibatch has loss 0 and gradient 0; AdamW still decays the
 * parameters.  MMF_EINVAL with nothing launched: a NULL required pointer, N < 1, batch outside 1..64,
 * a short ws. */
#define MMF_CLIP_TRAIN_PARAMS 655361  /* visual_projection.weight[512][768], text_projection.weight[512][512], logit_scale */
int64_t mmf_clip_train_ws_bytes(int batch);
int mmf_clip_train_epoch(const float* img_feat, const float* txt_feat, int N, const int32_t* perm, int batch,
                         double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                         int step0, float* params, float* exp_avg, float* exp_avg_sq, float* step_loss,
                         float* step_gnorm, float* grad_out, void* ws, int64_t ws_bytes, void* stream);

/* validate (train_clip_detective.py:236-273) on cached features: forward only, consecutive batches
 * in file order.  batch_loss fp32 [ceil(N / batch)]: the contrastive loss of each batch; row_cos
 * fp32 [N]: each pair's own cosine (calculate_accuracy's operand, :169-187).  ws and the errors as
 * the training call's. */
int mmf_clip_contrastive_eval(const float* img_feat, const float* txt_feat, int N, int batch, const float* params,
                              float* batch_loss, float* row_cos, void* ws, int64_t ws_bytes, void* stream);

/* A hyperparameter study of the same training (run_hyperparameter_tuning, train_clip_detective.py:427-454):
 * `trials` (1..MMF_CLIP_TRIALS_MAX) independent trainings side by side in the SAME six launches per
 * step (three per eval batch), the trial as a third grid dimension; synchronisation stays stream
 * order alone.  Every trial's results are bit-identical to mmf_clip_train_epoch /
 * mmf_clip_contrastive_eval called for it alone, whatever its neighbours are.
 *   img_feat, txt_feat: shared by all trials.
 *   params, exp_avg, exp_avg_sq fp32 [trials][MMF_CLIP_TRIAL_STRIDE] (a trial's
 *     MMF_CLIP_TRAIN_PARAMS values at the start of its slice); perm int32 [trials][N].
 *   batch, lr, weight_decay, max_norm, step0, active: HOST arrays [trials], read before the call
 *     returns.  Trials differ in batch size and so in steps: the call enqueues max ceil(N / batch[t])
 *     steps, and a trial past its last step takes no further part.  active[t] == 0 (active may be
 *     NULL: every trial is active): trial t takes no part at all -- not a byte of its params,
 *     moments, outputs or workspace is written, and its other entries are not read.
 *   step_loss, step_gnorm fp32 [trials][max_nsteps]; batch_loss fp32 [trials][max_nb]; row_cos
 *     fp32 [trials][N]: a trial writes its first ceil(N / batch[t]) entries of a row, no others.
 *   ws: ws_bytes >= mmf_clip_train_trials_ws_bytes(trials, 64) (0 for trials or batch_max out of
 *     range): one image of the single-trial workspace per trial.
 * MMF_EINVAL with nothing launched: trials outside 1..MMF_CLIP_TRIALS_MAX, N < 1, an active trial's
 * batch outside 1..64 or step0 < 0, max_nsteps / max_nb below an active trial's step count, a NULL
 * required pointer, a short ws, a device buffer off a 16-byte boundary. */
#define MMF_CLIP_TRIALS_MAX 16
#define MMF_CLIP_TRIAL_STRIDE 655364  /* MMF_CLIP_TRAIN_PARAMS rounded up to 4 floats */
int64_t mmf_clip_train_trials_ws_bytes(int trials, int batch_max);
int mmf_clip_train_epoch_trials(const float* img_feat, const float* txt_feat, int N, int trials, const int32_t* perm,
                                const int32_t* batch, const double* lr, const double* weight_decay,
                                const double* max_norm, const int32_t* step0, const int32_t* active, double beta1,
                                double beta2, double eps, float* params, float* exp_avg, float* exp_avg_sq,
                                float* step_loss, float* step_gnorm, int max_nsteps, void* ws, int64_t ws_bytes,
                                void* stream);
int mmf_clip_contrastive_eval_trials(const float* img_feat, const float* txt_feat, int N, int trials,
                                     const int32_t* batch, const int32_t* active, const float* params,
                                     float* batch_loss, float* row_cos, int max_nb, void* ws, int64_t ws_bytes,
                                     void* stream);

/* Host-input geometry on the device (misinfo_forensics.py:249-253 and the
 * CLIPImageProcessor the reference calls at :386-401): B decoded uint8 images (HWC, pixel_bytes =
 * 3 for RGB or 4 for RGBX -- Pillow's in-memory layout --, any size up to a 47x downscale)
 * concatenated in device memory at byte offsets[i] with sizes wh[2i] = width, wh[2i+1] = height
 * (host arrays) -> out_effnet uint8 [B,224,224,3] =
 * Image.resize((224,224), BILINEAR) and out_clip uint8 [B,224,224,3] = shortest edge -> 224 BICUBIC
 * + centre crop, both bit-exact with Pillow's resampler (either output may be NULL).  Returns after
 * the work on `stream` has completed; MMF_ERANGE (nothing launched) when an image needs more taps
 * per output pixel than the kernels hold (mmf_resize_supported). */
int mmf_resize_pil(mmf_handle* h, const uint8_t* src, const int64_t* offsets, const int32_t* wh, int B,
                   int pixel_bytes, uint8_t* out_effnet, uint8_t* out_clip, void* stream);

/* Device JPEG decode (the reference's Image.open(path).convert("RGB"),
 * misinfo_forensics.py:255-258, decodes through Pillow's libjpeg-turbo).  Host: marker parsing and
 * Huffman entropy decoding (the serial part); device: dequantisation, islow IDCT, fancy chroma
 * upsampling and YCbCr -> RGB, pixels bit-exact with Pillow's decoder.  Supported: 8-bit baseline /
 * extended sequential Huffman JPEGs with one scan, and progressive Huffman JPEGs (any scan script;
 * quantisation tables fixed before the first scan), grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0;
 * anything else returns MMF_EUNSUPPORTED (decode that file on the host).
 *
 * The exact range.  "Bit-exact with Pillow" holds while the integer IDCT stays where libjpeg's C code
 * (64-bit, range limit by table[v & 1023]), libjpeg-turbo's SIMD code (16-bit lanes, a saturating
 * clamp) and the device kernel (32-bit, the table's arithmetic) agree: for every block of the file
 * |coef * q| <= 32767, |pass-1 workspace| <= 32767 and -512 <= pass-2 output <= 511 (the table wraps
 * beyond: 512 -> 0).  Files an encoder writes are far inside; a file whose quantisation tables were
 * rewritten (8-bit or 16-bit, Pq = 1) need not be.  The header cannot tell, so mmf_jpeg_header
 * accepts such a file and the entropy decoders -- mmf_jpeg_entropy, mmf_jpeg_entropy_packed,
 * mmf_jpeg_stage_packed and the batch form's rcs[k] -- return MMF_EUNSUPPORTED for a file with any
 * block outside (outputs then hold no usable data, no staging room is reserved): decode that file on
 * the host.  mmf_jpeg_reconstruct itself does not check: its operands must come from those decoders
 * (or satisfy the same conditions).
 *
 * mmf_jpeg_header: host-only, no handle.  info[MMF_JPEG_INFO_LEN] = {width, height, ncomp, hmax, vmax,
 * bw0, bh0, bw1, bh1, bw2, bh2, blocks, 0...} (bw_c x bh_c = component c's MCU-padded block grid;
 * blocks = their sum = the int16[64] blocks mmf_jpeg_entropy writes).  Returns 0 if supported. */
#define MMF_JPEG_INFO_LEN 16
int mmf_jpeg_header(const uint8_t* data, int64_t nbytes, int32_t* info);
/* Host-only, thread-safe: quantised coefficients of every component as [bh_c][bw_c][64] int16
 * (natural order, components back to back) and the components' quantisation tables qt[c][64]
 * (natural order, uint16).  Replaces libjpeg's decode_mcu (jdhuff.c; progressive files: every scan
 * accumulated as jdphuff.c does). */
int mmf_jpeg_entropy(const uint8_t* data, int64_t nbytes, int16_t* coefs, uint16_t* qt);
/* Host-only, thread-safe: the same coefficients packed for the H2D copy (~2.8x fewer bytes than the
 * dense planes on photos): one record per block -- uint64 mask of its nonzero ZIGZAG positions, then
 * their int16 values in zigzag order, padded to 8 bytes -- in decode order after an all-zero record
 * at offset 0; block_off[b] = byte offset of block b's record (b in the dense layout's order, padding
 * blocks -> 0).  `out` must hold mmf_jpeg_packed_bound(blocks) bytes (MMF_ERANGE otherwise); *used =
 * bytes written.  This is the format mmf_jpeg_reconstruct reads. */
int64_t mmf_jpeg_packed_bound(int32_t blocks);
int mmf_jpeg_entropy_packed(const uint8_t* data, int64_t nbytes, uint8_t* out, int64_t cap, uint32_t* block_off,
                            uint16_t* qt, int64_t* used);
/* Host-only, thread-safe: mmf_jpeg_entropy_packed for a batch staged by several threads.  Decodes
 * into a per-thread scratch, reserves 8-aligned room by an atomic add on *cursor, sets *rec_off to it
 * and copies the records to dst + *rec_off -- or returns MMF_ERANGE (room still reserved) when they
 * do not fit in dst_cap bytes: grow dst and place that image again (mmf_jpeg_entropy_packed). */
int mmf_jpeg_stage_packed(const uint8_t* data, int64_t nbytes, uint8_t* dst, int64_t dst_cap, int64_t* cursor,
                          uint32_t* block_off, uint16_t* qt, int64_t* rec_off);
/* Host-only: mmf_jpeg_header over n files (null datas[k] -> MMF_EINVAL) on up to `nthreads` threads;
 * infos [n][MMF_JPEG_INFO_LEN], rcs[k] = file k's return code. */
int mmf_jpeg_header_batch(const uint8_t* const* datas, const int64_t* nbytes, int n, int32_t* infos, int32_t* rcs,
                          int nthreads);
/* Host-only: mmf_jpeg_stage_packed over n files on `nthreads` threads of its own (one C call per
 * chunk: no per-file interpreter work); file k's block offsets go to block_off + block_base[k], its
 * tables to qt + 192 k, its record offset to rec_off[k] and its status to rcs[k]. */
int mmf_jpeg_stage_packed_batch(const uint8_t* const* datas, const int64_t* nbytes, int n, uint8_t* dst,
                                int64_t dst_cap, int64_t* cursor, uint32_t* block_off, const int64_t* block_base,
                                uint16_t* qt, int64_t* rec_off, int nthreads, int32_t* rcs);
/* Device: B images' packed coefficients and tables -> uint8 RGBX pixels, bit-exact with Pillow's
 * decoder.  Every pointer is DEVICE memory: packed = the images' mmf_jpeg_entropy_packed records
 * (image i's at byte offset pk_off[i]), block_off uint32 = their block-offset tables concatenated
 * (image i's from index coef_blocks[i]), qt uint16 [B][3][64], infos int32 [B][MMF_JPEG_INFO_LEN]
 * (mmf_jpeg_header's), out_offsets int64 [B] (byte offset of image i's [h][w][4] RGBX pixels in
 * out_rgbx; X = 255), samples = scratch of 64 * sum(blocks) bytes (component sample planes, image i's
 * from 64 * coef_blocks[i]).  max_blocks / max_pixels = the largest blocks / width * height over the B
 * images (grid sizes).  Feeds mmf_resize_pil (pixel_bytes 4).  Asynchronous on `stream`. */
int mmf_jpeg_reconstruct(mmf_handle* h, const uint8_t* packed, const uint32_t* block_off, const int64_t* pk_off,
                         const uint16_t* qt, const int64_t* coef_blocks, const int32_t* infos, const int64_t* out_offsets,
                         int B, int max_blocks, int max_pixels, uint8_t* samples, uint8_t* out_rgbx, void* stream);

/* 1 if a width x height image fits mmf_resize_pil's tap budget in both geometries (bicubic CLIP:
 * shortest side <= ~5264 px; bilinear EfficientNet: either side <= ~10528 px), else 0.  Host-only,
 * no handle: callers route the few larger images to a host resampler. */
int mmf_resize_supported(int width, int height);

/* Truth-Vault (misinfo_forensics.py:214-246, 443-445): host fp32 [N, D=512] raw embeddings; rows
 * are L2-normalised once here instead of on every search call. */
int mmf_set_vault(mmf_handle* h, const float* host_vault, int N, int D);
/* The same with rows already L2-normalised by the caller: the Python host side normalises exactly
 * as the reference line does, in the vault's own dtype (numpy, misinfo_forensics.py:443-445 --
 * float16 vaults renormalise in float16; a zero row becomes NaN), and uploads the float32 result.
 * Replaces the previous vault and its title embeddings (their device memory is freed). */
int mmf_set_vault_normalized(mmf_handle* h, const float* host_vault_unit, int N, int D);
/* Pre-compute the CLIP text embeddings of the vault titles (used for text_similarity,
 * misinfo_forensics.py:467-484) from device ids/mask int32 [N, L<=77].  Synchronous. */
int mmf_set_vault_titles(mmf_handle* h, const int32_t* ids, const int32_t* mask, int N, int L, void* stream);

/* search_vault core (misinfo_forensics.py:443-464, 467-484): q fp32 [B, 512] unit image
 * embeddings; top-k (1 <= k <= N; on a vault of more than 16384 rows k <= 64 and
 * ceil(N / 16384) * k <= 16384) similarities fp32 [B, k] and indices
 * int32 [B, k] in np.argsort(sims)[-k:][::-1] order (descending; NaN rows first, exact ties by
 * descending index);
 * discrepancy fp32 [B] = top1 > thresh ? top1 : 0; optional text_emb fp32 [B, 512] unit caption
 * embeddings -> text_sim fp32 [B] = cos(caption, title[top1]) where top1 > thresh, else 0. */
int mmf_vault_topk(mmf_handle* h, const float* q_unit, int B, int k, float thresh, float* sims, int32_t* idx,
                   float* discrepancy, const float* text_emb, float* text_sim, void* stream);

/* fusion_verdict (misinfo_forensics.py:575-615): scores5 fp32 [B, 5] -> probs fp32 [B, 2]
 * (real, fake); verdict int32 [B] (fake > 0.5); confidence fp32 [B]; explanation rule index
 * int32 [B] of _generate_fallback_explanation (misinfo_forensics.py:742-765; 0 vault, 1 deepfake,
 * 2 ai, 3 misinfo, 4 clip, 5 default).  Any output except probs may be NULL. */
int mmf_fusion(mmf_handle* h, const float* scores5, int B, float* probs2, int32_t* verdict, float* confidence,
               int32_t* rule, void* stream);

/* FusionJudge training (train_fusion_judge.py:213-233): ONE epoch -- forward in training mode
 * (Linear(5,64)-ReLU-Dropout(p_drop)-Linear(64,32)-ReLU-Linear(32,2)), mean cross-entropy, backward
 * and torch.optim.AdamW (decoupled weight decay, bias correction by global step) for each of the
 * ceil(N / batch) minibatches -- in one launch.  No handle; asynchronous on `stream`.  All fp32;
 * every reduction has a fixed order, so results are bit-reproducible and do not depend on how an
 * epoch is split into launches.
 *   scores5 fp32 [N][5], labels int32 [N] (0 / 1), perm int32 [N]: minibatch s takes positions
 *     s*batch .. min(N, (s+1)*batch) - 1 of perm (the last may be short; its mean is over its own
 *     rows).  A perm entry outside [0, N) is clamped, so no input makes the kernel read out of bounds.
 *   keep uint64 [N] or NULL: keep[i] is the dropout mask of the row at POSITION i of the epoch order,
 *     bit j set = hidden unit j kept and scaled by 1 / (1 - p_drop); NULL = no dropout, no scaling.
 *   params, exp_avg, exp_avg_sq fp32 [MMF_FUSION_PARAMS], state-dict order, updated in place;
 *     step0 = optimizer steps already taken (step s corrects its bias with step0 + s + 1).
 *   step_loss fp32 [nsteps]: the minibatch's mean loss (train-mode logits, before its update);
 *   step_correct int32 [nsteps]: rows with argmax(logits) == label (a tie is class 0, as torch.max);
 *   grad_out fp32 [MMF_FUSION_PARAMS] or NULL: the gradient of the last minibatch.
 * MMF_EINVAL with nothing launched: a NULL required pointer, N < 1, batch outside 1..256, p_drop
 * outside [0, 1). */
#define MMF_FUSION_PARAMS 2530  /* 0.weight[64][5], 0.bias[64], 3.weight[32][64], 3.bias[32], 5.weight[2][32], 5.bias[2] */
int mmf_fusion_train_epoch(const float* scores5, const int32_t* labels, int N,
                           const int32_t* perm, const uint64_t* keep, float p_drop, int batch,
                           double lr, double beta1, double beta2, double eps, double weight_decay, int step0,
                           float* params, float* exp_avg, float* exp_avg_sq,
                           float* step_loss, int32_t* step_correct, float* grad_out, void* stream);

/* The whole text+image analyze() path for B pairs (misinfo_forensics.py:767-927) with the ViT
 * computed once per pair.  Inputs device: RoBERTa ids/mask [B, Lr], CLIP ids/mask [B, Lc],
 * img_effnet uint8 [B,224,224,3], img_clip uint8 [B,224,224,3] (may equal img_effnet).
 * Outputs device (all fp32 unless noted): scores5 [B,5] (ai, misinfo, deepfake, clip_similarity,
 * vault_discrepancy), text_sim [B], probs2 [B,2], verdict int32 [B], confidence [B], rule int32 [B],
 * top_sims [B,5], top_idx int32 [B,5].  Vault outputs are zero when no vault is set. */
int mmf_analyze_batch(mmf_handle* h, const int32_t* rob_ids, const int32_t* rob_mask, int Lr,
                      const int32_t* clip_ids, const int32_t* clip_mask, int Lc, const uint8_t* img_effnet,
                      const uint8_t* img_clip, int B, float* scores5, float* text_sim, float* probs2,
                      int32_t* verdict, float* confidence, int32_t* rule, float* top_sims, int32_t* top_idx,
                      void* stream);

/* analyze() for a batch of B posts where each has a text, an image or both
 * (misinfo_forensics.py:790-899), in one launch sequence; each tower runs only on the rows that
 * have its modality.
 *
 * mmf_mixed_plan: host-only, no handle, no device call.  modality uint8 [B] is a bit field per row
 * (1 = text, 2 = image, 3 = both) -> row_map int32 [B][3] = the row's position in the text list, the
 * image list and the both list (each list holds its rows in ascending batch order), -1 where the row
 * is not in the list; counts int32 [3] = {nT, nI, nC}, the lists' lengths.  MMF_EINVAL on NULL, B <= 0
 * or an entry that is 0 or > 3 (the reference's "Provide at least one of ..." error; nothing is
 * written past that row).
 *
 * mmf_analyze_mixed: inputs are COMPACTED device arrays: rob_ids / rob_mask int32 [nT, Lr] (the text
 * rows), img_effnet / img_clip uint8 [nI, 224, 224, 3] (the image rows; img_clip may be NULL =
 * img_effnet), clip_ids / clip_mask int32 [nC, Lc] (the rows with both).  A list whose count is 0 may
 * be NULL and its tower is not launched.  row_map is a DEVICE int32 [B][3] (mmf_mixed_plan's, copied
 * by the caller: no H2D copy happens inside the call); nT, nI, nC are passed by value and must
 * satisfy nT + nI - nC == B, nC <= nT, nC <= nI.  A map entry outside [0, n) of its list is treated
 * as absent, so no map makes a kernel read out of bounds.  Only the components the batch uses must
 * be loaded (text rows: RoBERTa + heads; image rows: EfficientNet + CLIP vision; both rows: + CLIP
 * text + fusion layer), else MMF_EINVAL.  B <= the reserved batch, lengths as mmf_analyze_batch.
 * Outputs: as mmf_analyze_batch, [B, ...] in batch order.  Per row:
 *   text only: ai, misinfo from RoBERTa; deepfake, clip_similarity, vault_discrepancy, text_sim and
 *              top_sims 0, top_idx -1; fake = clamp(misinfo, 0, 1)
 *   image only: deepfake from EfficientNet, vault top-5 / discrepancy of the ViT embedding; ai,
 *              misinfo, clip_similarity, text_sim 0; fake = clamp(max(deepfake, vault_discrepancy), 0, 1)
 *   both:      every output bit-identical to mmf_analyze_batch on that row
 *   single-modality rows: probs2 = (1 - fake, fake), verdict = fake > 0.5, confidence = verdict ?
 *              fake : 1 - fake; rule = the same cascade over the row's five scores in all cases. */
int mmf_mixed_plan(const uint8_t* modality, int B, int32_t* row_map, int32_t* counts);
int mmf_analyze_mixed(mmf_handle* h, const int32_t* row_map, int B, int nT, int nI, int nC,
                      const int32_t* rob_ids, const int32_t* rob_mask, int Lr, const int32_t* clip_ids,
                      const int32_t* clip_mask, int Lc, const uint8_t* img_effnet, const uint8_t* img_clip,
                      float* scores5, float* text_sim, float* probs2, int32_t* verdict, float* confidence,
                      int32_t* rule, float* top_sims, int32_t* top_idx, void* stream);

/* Per-kernel timing for roofline accounting: while profiling is on, every kernel launch of the
 * forward calls is bracketed by two hipEvents on its stream.  mmf_profile_end synchronises and
 * aggregates per kernel kind (arrays of >= 16 entries): launch counts, summed device ms, summed
 * ALGORITHMIC flops and HBM bytes; returns the number of kinds.  Names via mmf_profile_kind_name. */
int mmf_profile_begin(mmf_handle* h);
int mmf_profile_end(mmf_handle* h, int max_kinds, int* counts, double* ms, double* flops, double* bytes);
const char* mmf_profile_kind_name(int kind);

/* Run-time options.  Defaults are read once per process from MMF_<NAME> environment variables
 * (e.g. MMF_GEMM_KLOOP), copied into every handle at mmf_create and changed with mmf_set_option
 * (h = NULL: the process defaults, used by the handle-less ops below and by handles created
 * afterwards).  The library's list is exactly the following (mmf_option_name enumerates it; the CPU
 * test tests/test_capi_cpu.py::test_header_options_match_library ties the two):
 *   "concurrent"     1: towers of mmf_analyze_batch on concurrent streams (0: one stream)
 *   "fuse_stem"      1: EfficientNet stem fused into the stage-1 depthwise conv
 *   "fuse_expand"    1: 1x1 expand fused into the depthwise conv (stages 2 - 4.3)
 *   "gemm_splitk"    1: split-K on the skinny-M (M <= 512) GEMM path
 *   "gemm_config"   -1: automatic GEMM tile choice; c >= 0 forces instantiation c (A/B tools)
 *   "gemm_group_m"   0: persistent GEMM tile order (g > 0: grouped by g row panels)
 *   "text_hilo"     -1: RoBERTa stream layout: -1 chosen at weight-load time from the LayerNorm
 *                       bound (fp16 hi + lo if max_c |beta_c| + sqrt(767) |gamma_c| > 64, fp16 alone
 *                       otherwise), 0 fp16, 1 fp16 hi + lo, 2 precise mode (fp32 stream, LayerNorm,
 *                       attention and branch outputs; GEMM operands per "text_prec_mask").  2 needs
 *                       the precise weights (packed unless the layout was pinned to 0 / 1 at load)
 *   "text_prec_mask" 255: precise mode operands per GEMM kind k (0 QKV, 1 out-proj, 2 FFN-1, 3 FFN-2):
 *                       bit k = hi / lo activations ([A_hi | A_lo] x [W_hi | W_hi], K = 2 in), bit
 *                       k + 4 = also W_lo (+ A_hi x W_lo, K = 3 in: ~22-bit operands); neither = fp16
 *   "effnet_fp32"    0: 1 = EfficientNet tower with fp32 activations, fp32-MFMA 1x1 convs and
 *                       precise SiLU (checkpoints whose logits amplify fp16 storage rounding)
 *   "clip_res16"     1: CLIP pre-LN residual streams in fp16 (0: fp32)
 *   "lazy_ln"        1: CLIP encoder LayerNorms folded into the GEMM epilogues
 *   "pw32_mfma"      5: fp32 tower's 1x1 convs (0 fp32-FMA VALU, 1 / 2 fp32 MFMA with 1 / 3 K-chunks
 *                       prefetched, 3 / 4 / 5 whole-row tiles; bit-identical)
 *   "effnet_chunks"  2: mmf_effnet_forward batch chunks on concurrent streams
 *   "dw_cw32"        1: 32-channel groups for the standalone depthwise convs
 *   "diag_skip"      0: diagnostic bitmask of towers mmf_analyze_batch leaves out (2 EfficientNet,
 *                       4 CLIP text, 8 ViT, ...; measurement only)
 *   "qkv_attn"       1: RoBERTa L = 128: attention in the QKV GEMM's epilogue
 *   "clip_qkv_attn"  1: CLIP towers (lazy LN, L <= 128): attention in the QKV consumer GEMM's epilogue
 *                       (bit-identical to 0; 2 = ViT only, 4 = text tower only)
 *   "vault_ref"      0: diagnostic: vault similarities on the VALU kernel, top-k by full sort (the
 *                       reference kernels the production MFMA / register top-k kernels equal bit for bit)
 *   "vault_fused"    2: vault search without the [B, N] similarity matrix (fused similarity + top-k
 *                       kernel, bit-identical results): 0 the two-kernel path, 1 fused wherever
 *                       top_k <= 8, 2 fused iff the vault has more than 16384 rows
 *   "mt_enqueue"    64: batches of <= this many pairs: towers enqueued by host threads side by side
 *   "last_q1"        1: compact last encoder layers (bit 1 RoBERTa, bit 2 CLIP towers)
 *   "after_text"    12: towers of the concurrent step that start once RoBERTa is done (bitmask as
 *                       diag_skip)
 * The defaults are the measured best; with them a row's results do not depend on the
 * batch it runs in (tests/test_gpu_parity.py).  Read-only names for mmf_get_option with a handle:
 * "text_hilo_effective" (the RoBERTa layout in use) and "text_precise_packed" (bitmask of the GEMM
 * kinds whose precise-mode weights are packed, bits 0-3 as "text_prec_mask"; setting it to a subset
 * releases the others' weights). */
const char* mmf_option_name(int i); /* i-th option name, NULL past the end */
int mmf_set_option(mmf_handle* h, const char* name, int value);
int mmf_get_option(mmf_handle* h, const char* name, int* value);
/* Device bytes currently owned by the handle (weights, workspaces, vault). */
int64_t mmf_device_bytes(mmf_handle* h);

/* Low-level vault search over caller-owned device memory (no handle): what mmf_vault_topk computes, by
 * the fused similarity + top-k kernels, for any bank of unit rows.  q_unit fp32 [B, D], bank_unit fp32
 * [N, D]; D must be 512 and k in 1..8 (k > N pads slots N.. with similarity -inf and index -1);
 * outputs as mmf_vault_topk, discrepancy at discrepancy[b * disc_stride]; title_bank fp32 [N, D] or
 * NULL.  ws: mmf_vault_search_ws_bytes(B, k, nblocks) bytes of device scratch.  nblocks = vault
 * partitions (blocks per 64 queries, each walking a contiguous range of 64-row tiles; 0 = automatic,
 * at most 256); the result does not depend on it. */
int64_t mmf_vault_search_ws_bytes(int B, int k, int nblocks);
int mmf_vault_search_rows(const float* q_unit, const float* bank_unit, int B, int N, int D, int k, float thresh,
                          float* sims, int32_t* idx, float* discrepancy, int disc_stride, const float* text_emb,
                          const float* title_bank, float* text_sim, void* ws, int64_t ws_bytes, int nblocks,
                          void* stream);

/* Low-level op exported for unit tests of the GEMM kernel: C = act(A @ W^T + bias) + residual.
 * A fp16 [M,K] (lda), W fp16 [N,K] (ldw), bias fp32 [N] or NULL, residual fp32 [M,N] (ldc) or NULL,
 * act 0 none 1 gelu-erf 2 quick_gelu 3 silu 4 relu; outputs fp32 (c32) and/or fp16 (c16) [M,N] ldc. */
int mmf_gemm_f16(const void* A, int lda, const void* W, int ldw, const float* bias, const float* residual,
                  float* c32, void* c16, int ldc, int M, int N, int K, int act, void* stream);

/* The same with the EfficientNet operands of the 1x1 convolutions: fp16 residual res16 [M,N] (ldc)
 * and a per-(image, k) fp32 scale ascale [M / rows_per_batch, K] applied to A (SE excitation). */
int mmf_gemm_f16_ex(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res16,
                     const float* ascale, int rows_per_batch, void* c16, int ldc, int M, int N, int K, int act,
                     void* stream);

/* The RoBERTa precise mode's FFN-1 epilogue (gemm.hip epi 4), exported for its bit-identity test:
 * out = act(A @ W^T + bias) written as the next GEMM's split operand row -- c16[m*ldc + n] = fp16(out)
 * and, with split_lo, c16[m*ldc + N + n] = fp16(out - fp16(out)), c16[m*ldc + 2N + n] = fp16(out)
 * (ldc >= 3N).  bias fp32 [N] (required), act 1 (gelu-erf) only; persistent-tile shapes only
 * (K % 64 == 0, N % 8 == 0), else MMF_EINVAL. */
int mmf_gemm_f16_split(const void* A, int lda, const void* W, int ldw, const float* bias, void* c16, int ldc, int M,
                       int N, int K, int act, int split_lo, void* stream);

/* Low-level attention op for tests: qkv fp16 [B*L, 3*H*64] (q|k|v), mask int32 [B,L] or NULL,
 * causal 0/1 -> out fp16 [B*L, H*64].  L <= 512. */
int mmf_attention_f16(const void* qkv, const int32_t* mask, void* out, int B, int L, int H, int causal,
                       void* stream);

/* Low-level ops exported for unit tests of the fp16 EfficientNet kernels (tests/test_gpu_effnet_kernels.py).
 * No handle; every pointer is a device pointer; work is enqueued on `stream`.  Activations are fp16
 * NHWC ([B][H][W][C]), weights and biases fp32 with BatchNorm already folded.  A shape a kernel does
 * not support is MMF_EINVAL, decided on the host before anything is launched.
 *
 * Depthwise k x k convolution (k 3 or 5, stride 1 or 2, zero padding (k - 1) / 2) + SiLU:
 *   in [B][H][W][C] -> out [B][Ho][Wo][C], Ho = (H - 1) / stride + 1; w [C][k*k], bias [C];
 *   pool_part [B][nchunks][C] fp32 = per output tile (row-major tiles of edge T, the largest divisor of
 *   Ho up to 16 / 8 for stride 1 / 2) the sum of the unrounded outputs; nchunks = mmf_dwconv_nchunks
 *   (host arithmetic only; MMF_EINVAL on a bad shape).  flags bit 0: compile-time tile geometries where
 *   one exists; bit 3: 32-channel groups where C % 32 == 0.  C % 48 == 0 or C % 32 == 0; B <= 65535;
 *   H * W * C < 2^30. */
int mmf_dwconv_nchunks(int H, int W, int C, int stride);
int mmf_dwconv_f16(const void* in, const float* w, const float* bias, void* out, float* pool_part, int B, int H, int W,
                   int C, int k, int stride, int flags, void* stream);
/* The same behind a fused 1x1 expand + SiLU: x fp16 [B][H][W][cin], we fp16 [C][cin], be fp32 [C]; the
 * expanded activation (rounded to fp16, as the separate GEMM stores it) feeds the depthwise conv above.
 * cin % 8 == 0, C % 48 == 0, cin <= 64 (k = 5) or <= 96 (k = 3), (k, stride, ceil(cin / 32)) one of
 * (3,2,1) (3,1,1) (5,2,1) (5,1,2) (3,2,2) (3,1,3), input tile edge (T - 1) stride + k <= 19.
 * ct 1: compile-time geometries where one exists. */
int mmf_expand_dw_f16(const void* x, int cin, const void* we, const float* be, const float* w, const float* bias,
                      void* out, float* pool_part, int B, int H, int W, int C, int k, int stride, int ct, void* stream);
/* Squeeze-excitation: pooled[c] = inv_hw * sum_j pool_part[b][j][c]; s1 = SiLU(w1 pooled + b1), w1 [Csq][C];
 * scale [B][C] = sigmoid(w2t^T s1 + b2), w2t [Csq][C] (fc2's weight transposed).  precise 1: the SiLU by
 * expf and a division (the fp32 tower's).  C <= 1280, Csq <= 64. */
int mmf_se_f32(const float* pool_part, int nchunks, float inv_hw, const float* w1, const float* b1, const float* w2t,
               const float* b2, float* scale, int B, int C, int Csq, int precise, void* stream);
/* Stem: ToTensor + Normalize (ImageNet) -> conv 3x3 stride 2 pad 1, 3 -> 32 + SiLU -> out fp16 [B][112][112][32].
 * Exactly one of img_u8 (uint8 [B][224][224][3]) and x_f32_nchw (normalised fp32 [B][3][224][224]) is
 * non-NULL; w [32][3][3][3], bias [32]. */
int mmf_effnet_stem_f16(const uint8_t* img_u8, const float* x_f32_nchw, const float* w, const float* bias, void* out,
                        int B, void* stream);
/* The stem fused into the stage-1 depthwise conv (3x3, stride 1, 32 channels): ws / bs the stem's, wd [32][9] /
 * bd [32] the depthwise conv's; out fp16 [B][112][112][32], pool_part [B][49][32] (16 x 16 tiles). */
int mmf_effnet_stem_dw_f16(const uint8_t* img_u8, const float* x_f32_nchw, const float* ws, const float* bs,
                           const float* wd, const float* bd, void* out, float* pool_part, int B, void* stream);
/* Global average pool + Linear(C, 2) + softmax: x fp16 [B][HW][C], w [2][C], b [2] -> logits [B][2] and / or
 * score[b * score_stride] = softmax(logits[b])[1] (either may be NULL, not both).  C % 8 == 0. */
int mmf_gap_classifier_f16(const void* x, int HW, int C, const float* w, const float* b, float* logits, float* score,
                           int score_stride, int B, void* stream);

/* Low-level ops exported for unit tests of the fp32 EfficientNet tower's kernels (option effnet_fp32;
 * tests/test_gpu_effnet32_kernels.py).  No handle; every pointer is a device pointer; activations, weights
 * and biases are fp32, activations NHWC; work is enqueued on `stream`.  Null, shape and alignment checks run on
 * the host; anything unsupported is MMF_EINVAL with nothing launched.
 *
 * pw32_variant (host arithmetic only): the kernel a 1x1 convolution of M rows, N outputs, K inputs runs under
 *   pw32_mfma mode `mfma` (0..5): returns 0 = the VALU kernel, 1 = pw32m<D>, 2 = pw32r<NF, D> over column tiles
 *   of NC, and writes {D, NF, NC} to d_nf_nc (nullable; NF = 0 for kinds 0 and 1, D = 0 for kind 0).
 * pw32: C [M][N] = act((A [M][K] .* ascale[m / rows_per_image][K]) W^T + bias) (+ res [M][N]); W [N][K], bias [N]
 *   (required); ascale and res nullable; act 0 (none) or 3 (SiLU, by expf and a division); N % 4 == 0,
 *   K % 4 == 0, rows_per_image >= 1 with ascale; every pointer 16-byte aligned.
 * dw32: depthwise k x k (3 or 5, stride 1 or 2, zero padding (k - 1) / 2) + SiLU: in [B][H][W][C] -> out
 *   [B][Ho][Wo][C], Ho = (H - 1) / stride + 1; w TAP-MAJOR [k*k][C], bias [C]; C % 4 == 0, B * H * W * C < 2^32.
 * sum32: part [B][nchunks][C] = per channel the sum of x [B][HW][C] over the pixels [j HW / nchunks,
 *   (j + 1) HW / nchunks) of chunk j, in the fixed order csrc/effnet_f32.hip documents; C % 16 == 0,
 *   1 <= nchunks <= min(HW, 65535), HW <= 2^20, B <= 65535.
 * gap32: global average pool + Linear(C, 2) + softmax: x [B][HW][C], w [2][C], b [2] -> logits [B][2] and / or
 *   score[b * score_stride] = softmax(logits[b])[1] (either may be NULL, not both); score_stride >= 1.
 * stem32: mmf_effnet_stem_f16's operands -> out fp32 [B][112][112][32]; from uint8 pixels the normalisation is
 *   (u / 255 - mean) / std with two divisions, as torchvision evaluates it.  B <= 65535. */
int mmf_pw32_variant(int M, int N, int K, int mfma, int32_t* d_nf_nc);
int mmf_pw32_f32(const float* A, const float* W, const float* bias, const float* ascale, int rows_per_image,
                 const float* res, float* C, int M, int N, int K, int act, int mfma, void* stream);
int mmf_dw32_f32(const float* in, const float* w_tapmajor, const float* bias, float* out, int B, int H, int W, int C,
                 int k, int stride, void* stream);
int mmf_sum32_f32(const float* x, int B, int HW, int C, int nchunks, float* part, void* stream);
int mmf_gap32_f32(const float* x, int HW, int C, const float* w, const float* b, float* logits, float* score,
                  int score_stride, int B, void* stream);
int mmf_effnet_stem32_f32(const uint8_t* img_u8, const float* x_f32_nchw, const float* w, const float* bias,
                          float* out_f32, int B, void* stream);

/* Low-level ops exported for unit tests of the transformer towers' kernels (tests/test_gpu_transformer_kernels.py):
 * norm.hip, precise.hip, the one-query attention and the split-K skinny GEMM.  No handle; every pointer
 * is a device pointer; work is enqueued on `stream`.  "fp16" buffers are void*.  Null, shape and alignment
 * checks run on the host; what a kernel does not support is MMF_EINVAL with nothing launched.
 *
 * Row kernels: one row of C in {512, 768} columns per wave; every row stride >= C and a multiple of 4.
 *   layernorm: y = LN(x [+ add]) g + b -> y32 and / or y16.
 *   add_ln_f32: s = x + y (y fp16); s32 = s, o32 = LN(s) (both nullable, row stride ldx, may alias x), o16 = LN(s).
 *   add_ln_f16: the same on an fp16 stream: s16 = fp16(s) (nullable, may alias x16), o16 = LN of the stored s16.
 *   add_ln_hilo: (hi, lo) = split(LN((hi + lo) + y)) in place, C = 768; lo NULL = hi alone; ovf (nullable,
 *     needs L > 0): ovf[row / L] = 1 for a row with non-finite statistics.
 *   hilo_rows: out [B][C] fp32 = hi[b * row_stride] + lo[b * row_stride] (lo nullable); C, row_stride % 4 == 0.
 *   layernorm_split3: x = LN(x + add) in place [rows][768], s3 [rows][3 * 768] = [hi | lo | hi] of it
 *     (hi = fp16(x), lo = fp16(x - hi); with_lo 0: the first third only). */
int mmf_layernorm_f32(const float* x, int ldx, const float* add, int ldadd, const float* g, const float* b, float eps,
                      float* y32, int ldy32, void* y16, int ldy16, int rows, int C, void* stream);
int mmf_add_ln_f32(const float* x, int ldx, const void* y, int ldy, const float* g, const float* b, float eps,
                   float* s32, float* o32, void* o16, int ldo, int rows, int C, void* stream);
int mmf_add_ln_f16(const void* x16, int ldx, const void* y, int ldy, const float* g, const float* b, float eps,
                   void* s16, void* o16, int ldo, int rows, int C, void* stream);
int mmf_add_ln_hilo_f16(void* hi, void* lo, int ld, const void* y, int ldy, const float* g, const float* b, float eps,
                        int rows, int C, int32_t* ovf, int L, void* stream);
int mmf_hilo_rows_f32(const void* hi, const void* lo, int row_stride, float* out, int B, int C, void* stream);
int mmf_layernorm_split3_f32(float* x, const float* add, const float* g, const float* b, float eps, void* s3,
                             int with_lo, int rows, int C, void* stream);
/* Embeddings.  RoBERTa: position id = pad_id + (number of non-pad ids up to and including t) for a non-pad
 *   id, pad_id for a pad; row = LN(word[id] + type0 + pos[position id]) written as the split stream xb (hi) +
 *   xlo (lo, nullable), or as fp32 x32 when that is non-NULL; ovf (nullable, [B]) as above.  H = 768, L <= 512;
 *   every id must index word, pos needs pad_id + L + 1 rows.
 * CLIP text: x = tok[id] + pos[t] stored as fp32 x or fp16 x16 (exactly one), then xb = LN(stored x) fp16, or,
 *   with st (float2 [B * L]) non-NULL, st[row] = (mean, sum of squared deviations) of the stored row and xb is
 *   not written.  H = 512.
 * CLIP vision: row t of image b = pre-LN((t == 0 ? cls : patches[b * 49 + t - 1]) + pos[t]) stored to x / x16,
 *   then xb / st as for the text embeddings; 50 rows of 768 per image.
 * im2col: img uint8 [B][224][224][3] (8-byte aligned) -> A fp16 [B * 49][3072], column c * 1024 + ky * 32 + kx
 *   of patch p = ((img / 255) - mean_c) / std_c with CLIP's constants. */
int mmf_roberta_embed_f32(const int32_t* ids, const float* word, const float* pos, const float* type0, const float* g,
                          const float* b, float eps, void* xlo, void* xb, float* x32, int32_t* ovf, int B, int L, int H,
                          int pad_id, void* stream);
int mmf_clip_text_embed_f32(const int32_t* ids, const float* tok, const float* pos, const float* g, const float* b,
                            float eps, float* x, void* x16, void* xb, void* st, int B, int L, int H, void* stream);
int mmf_clip_vision_assemble_f32(const float* patches, const float* cls, const float* pos, const float* pre_g,
                                 const float* pre_b, const float* ln1_g, const float* ln1_b, float eps, float* x,
                                 void* x16, void* xb, void* st, int B, void* stream);
int mmf_clip_im2col_f16(const uint8_t* img, void* A, int B, void* stream);
/* Pooling.  eos_index: out[b] = first t with ids[b][t] == eos_id (0 if none), or, with eos_id == 2, the first
 *   position of the largest id; L <= 1024.  gather_ln: out16 / out32 [B][C] = LN(x[b * L + (idx ? idx[b] : 0)]),
 *   C in {512, 768}.  gather_rows2: the same rows of a16 (fp16, nullable: o16 untouched) -> o16 and of a32 (fp32)
 *   or a32h (fp16), exactly one, -> o32; C % 4 == 0.  l2norm: rows of x [B][C] scaled to unit length in place,
 *   C % 64 == 0. */
int mmf_eos_index_i32(const int32_t* ids, int32_t* out, int B, int L, int eos_id, void* stream);
int mmf_gather_ln_f32(const float* x, const int32_t* idx, int L, const float* g, const float* b, float eps, void* out16,
                      float* out32, int B, int C, void* stream);
int mmf_gather_rows2(const void* a16, const float* a32, const void* a32h, const int32_t* idx, int L, int C, void* o16,
                     float* o32, int B, void* stream);
int mmf_l2norm_f32(float* x, int B, int C, void* stream);
/* RoBERTa precise mode.  split3: out [rows][3C] = [hi | lo | hi] of x [rows][ldx] fp32 (with_lo 0: the first
 *   third only); C, ldx % 4 == 0.  attention32: fp32 attention, head dim 64, over qkv fp32 [B * L][ld] (q at
 *   h * 64, k at koff + h * 64, v at voff + h * 64; all % 4 == 0), key mask int32 [B][L] or NULL -> exactly one of
 *   out fp32 [B * L][ldo] and out3 fp16 [B * L][3 * H * 64] = [hi | lo | hi] of the same values. */
int mmf_split3_f32(const float* x, int ldx, void* out, int rows, int C, int with_lo, void* stream);
int mmf_attention32_f32(const float* qkv, int ld, int koff, int voff, const int32_t* mask, float* out, int ldo,
                        void* out3, int with_lo, int B, int L, int H, void* stream);
/* One query per sequence (the compact last layer): q fp32 [B][ldq] (head h at h * 64) over the keys / values of
 * qkv fp16 [B * L][ld] (columns koff + h * 64 / voff + h * 64); a key is excluded by mask 0 (int32 [B][L],
 * nullable) or by lying past qpos[b] (nullable) -> out fp16 row b at out + b * ldo.  L <= 512; ldq % 4 == 0;
 * ld, koff, voff % 8 == 0. */
int mmf_attention_q1_f16(const float* q, int ldq, const void* qkv, int ld, int koff, int voff, const int32_t* mask,
                         const int32_t* qpos, void* out, int ldo, int B, int L, int H, void* stream);
/* mmf_gemm_f16 with the skinny-M path's split-K workspace: ws fp32 of ws_elems floats (nullable).  With M <= 512,
 * N > 64 and S = mmf_gemm_splitk_factor(M, N, K, ldc) > 1, a workspace of >= S * M * N floats makes the GEMM
 * run as S slices of K reduced in slice order; a smaller one (or process option gemm_splitk = 0) gives the
 * unsplit kernel.  At most one of res32 (fp32 [M][N] ldc, may alias c32) and res16 (fp16 [M][N] ldc). */
int mmf_gemm_splitk_factor(int M, int N, int K, int ldc);
int mmf_gemm_f16_splitk(const void* A, int lda, const void* W, int ldw, const float* bias, const float* res32,
                        const void* res16, float* c32, void* c16, int ldc, int M, int N, int K, int act, float* ws,
                        int64_t ws_elems, void* stream);
/* The plain (epilogue 0) GEMM with every operand and stride independent: c = act((A * ascale) @ W^T + bias) + residual.
 * A fp16 [M][K] lda, W fp16 [N][K] ldw, bias fp32 [N] (nullable), at most one of res32 fp32 / res16 fp16 [M][N] ldr
 * (ldr >= N, ldr % 4 == 0; res32 may alias c32), ascale fp32 [ceil(M / rows_per_batch)][K] (nullable; row m of A is
 * scaled by row m / rows_per_batch and rounded to fp16), c32 fp32 / c16 fp16 [M][N] ldc (at least one).  No split-K
 * workspace.  The process options apply; *config_out (nullable) receives the instantiation that runs for exactly
 * these arguments (a forced gemm_config that is inapplicable gives the automatic one).  K % 8, N % 4, lda % 8,
 * ldw % 8, ldc % 4 == 0, act 0..4, 16-byte aligned base pointers, else MMF_EINVAL with nothing launched. */
int mmf_gemm_f16_raw(const void* A, int lda, const void* W, int ldw, const float* bias, const float* res32,
                     const void* res16, int ldr, const float* ascale, int rows_per_batch, float* c32, void* c16,
                     int ldc, int M, int N, int K, int act, int* config_out, void* stream);
/* The lazy-LayerNorm producer (gemm.hip epi 2): c16 = fp16(A @ W^T + bias + res16), res16 / c16 fp16 [M][ldc] (the
 * same buffer: in place), and ln_out float2 [M][ceil(N / tn)] = per row and block of tn = mmf_gemm_ln_tn(M, N, K)
 * consecutive columns the (mean, sum of squared deviations) of the stored values.  K % 64 == 0, K >= 192,
 * ceil(N / tn) <= 8, else MMF_EINVAL. */
int mmf_gemm_ln_tn(int M, int N, int K);
int mmf_gemm_f16_ln_producer(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res16,
                             void* c16, int ldc, void* ln_out, int M, int N, int K, void* stream);
/* The lazy-LayerNorm consumer (gemm.hip epi 1): A fp16 [M][K] = raw stream rows s, W fp16 [N][K] = W diag(gamma),
 * ln_u fp32 = its row sums, bias fp32 = b + W beta (both N + 256 entries: the tile's 256 columns are read whole),
 * ln_in float2 [rows][P] = per row (mean, sum of squared deviations) over consecutive blocks of tn columns
 * (rows padded to a multiple of 256; P * tn >= K, P <= 8) -> c16 = act(rstd (s W^T - mean u) + bias), act 0 / 1 /
 * 2, with mean / rstd combined from the partials (Chan).  Padding may hold anything.  K % 64 == 0, K >= 192. */
int mmf_gemm_f16_ln_consumer(const void* A, int lda, const void* W, int ldw, const float* bias, const void* ln_in,
                             int P, int tn, const float* ln_u, float eps, void* c16, int ldc, int M, int N, int K,
                             int act, void* stream);
/* The QKV GEMM with the attention of its rows in the epilogue (gemm.hip epi 3): A fp16 [M][K] = sequences of 128
 * rows, W fp16 [N][K] / bias [N] the fused QKV with rows interleaved per head ([q_h; k_h; v_h] = 192 rows for head
 * h), amask int32 [M / 128][128] (1 keep) or NULL -> ctx fp16 [M][ldc], head h at columns 64 h: bit-identical to
 * mmf_gemm_f16 on the same operands, de-interleaved, followed by mmf_attention_f16.  M % 128 == 0, N % 192 == 0,
 * K % 64 == 0, K >= 192, ldc >= N / 3, else MMF_EINVAL. */
int mmf_gemm_f16_attn(const void* A, int lda, const void* W, int ldw, const float* bias, const int32_t* amask, void* ctx,
                      int ldc, int M, int N, int K, void* stream);
/* The lazy-LayerNorm consumer with the attention of its rows in the epilogue (gemm.hip epi 5): the operands of
 * mmf_gemm_f16_ln_consumer with W / ln_u / bias rows interleaved per head as for mmf_gemm_f16_attn, A = sequences of L
 * rows (16 <= L <= 128, M % L == 0), amask int32 [M / L][L] (1 keep) or NULL, causal 0 / 1 -> ctx fp16 [M][ldc], head
 * h at columns 64 h: bit-identical to mmf_gemm_f16_ln_consumer (256 x 192 tiles) on the same operands, de-interleaved,
 * followed by mmf_attention_f16.  N % 192 == 0, K % 64 == 0, K >= 192, P <= 8, P * tn >= K, ldc >= N / 3, else
 * MMF_EINVAL with nothing written. */
int mmf_gemm_f16_ln_attn(const void* A, int lda, const void* W, int ldw, const float* bias, const void* ln_in, int P,
                         int tn, const float* ln_u, float eps, const int32_t* amask, int L, int causal, void* ctx,
                         int ldc, int M, int N, int K, void* stream);

/* Low-level ops exported for unit tests of the closing fp32 kernels (csrc/misc.hip; tests/test_gpu_misc_kernels.py)
 * and of the vault's stages (csrc/vault.hip; tests/test_gpu_vault_kernels.py).  No handle; every pointer is a device
 * pointer; work is enqueued on `stream`.  Null, shape, stride and alignment checks run on the host; what a launcher
 * does not support is MMF_EINVAL with nothing launched.
 *
 * text_heads: the two Linear(768,256)-ReLU-Linear(256,2) heads on rows x[b * row_stride .. + 768) (row_stride >= 768).
 *   w1a_t / w1m_t are the first layers TRANSPOSED, [768][256], as the kernel reads them; b1 [256], w2 [2][256], b2 [2].
 *   ai_logits / mi_logits [B][2] and scores (scores[b * score_stride + 0] = softmax(ai)[1], [+ 1] = softmax(misinfo)[1],
 *   score_stride >= 2) are nullable, not all three.  ovf (nullable, int32 [B]): a row with ovf[b] != 0 gets NaN.
 * text_cls_rows: out [B][768] = the same rows, NaN where ovf[b] != 0; row_stride % 4 == 0, x and out 16-byte aligned.
 * fusion_raw: the FusionJudge MLP 5 -> 64 -> 32 -> 2 with ReLUs on x5 [B][5], weights as PyTorch stores them (w0
 *   [64][5], w3 [32][64], w5 [2][32]) -> probs [B][2] = softmax, verdict = probs[1] > 0.5, conf = the verdict's
 *   probability, rule = the explanation cascade on x5 (verdict, conf, rule nullable).
 * rowdot: out[b * ostride] = dot(a[b], c[b]) over C columns.
 * mixed_finish_raw: mmf_analyze_mixed's last kernel; the arguments are csrc/kernels.h MixedFinishArgs field by field.
 * vault_sims: S [B][N] = q [B][D] . v [N][D]^T, each element one fp32 fma chain over k = 0 .. D - 1; D % 64 == 0, q, v
 *   and S 16-byte aligned; ref 0 = the fp32-MFMA kernel, 1 = the VALU kernel it is bit-identical to.
 * vault_topk: the top k of each row of a caller-supplied S [B][N] (value descending, NaN first, ties by descending
 *   index; slots past N hold (-inf, -1)) -> sims / idx [B][k], disc[b * disc_stride] = the top-1 of a hit (> thresh,
 *   not NaN) else 0, tsim[b] = dot(temb[b], title[top-1]) over D columns on a hit with both present, else 0; every
 *   output nullable, not all.  k <= 8 runs the register kernels, k > 8 (or ref = 1 with N <= 16384) the LDS sort,
 *   which needs max(N, k) <= 16384.
 * vault_sort_cand: the final ranking of cs / cidx [chunks][B][k] per-chunk results (chunk-local indices, -1 = an empty
 *   slot; global index = chunk * chunk_rows + local), chunks * k <= 16384, with the same outputs. */
int mmf_text_heads_f32(const float* x, int row_stride, const float* w1a_t, const float* b1a, const float* w2a,
                       const float* b2a, const float* w1m_t, const float* b1m, const float* w2m, const float* b2m,
                       float* ai_logits, float* mi_logits, float* scores, int score_stride, const int32_t* ovf, int B,
                       void* stream);
int mmf_text_cls_rows_f32(const float* x, int row_stride, const int32_t* ovf, float* out, int B, void* stream);
int mmf_fusion_raw_f32(const float* x5, const float* w0, const float* b0, const float* w3, const float* b3,
                       const float* w5, const float* b5, float* probs, int32_t* verdict, float* conf, int32_t* rule,
                       int B, void* stream);
int mmf_rowdot_f32(const float* a, const float* c, float* out, int ostride, int B, int C, void* stream);
int mmf_mixed_finish_raw(const int32_t* row_map, int B, int nT, int nI, int nC, const float* text2,
                         const float* deepfake, const float* v_emb, const float* t_emb, const float* c_sims,
                         const int32_t* c_idx, const float* c_disc, const float* title, float thresh, const float* w0,
                         const float* b0, const float* w3, const float* b3, const float* w5, const float* b5,
                         float* scores5, float* text_sim, float* probs, int32_t* verdict, float* conf, int32_t* rule,
                         float* top_sims, int32_t* top_idx, void* stream);
int mmf_vault_sims_f32(const float* q, const float* v, float* S, int B, int N, int D, int ref, void* stream);
int mmf_vault_topk_f32(const float* S, int B, int N, int k, float thresh, float* sims, int32_t* idx, float* disc,
                       int disc_stride, const float* temb, const float* title, int D, float* tsim, int ref,
                       void* stream);
int mmf_vault_sort_cand_f32(const float* cs, const int32_t* cidx, int chunks, int chunk_rows, int B, int k,
                            float thresh, float* sims, int32_t* idx, float* disc, int disc_stride, const float* temb,
                            const float* title, int D, float* tsim, void* stream);

/* Test-only: the block arithmetic of mmf_jpeg_roundtrip_u8 on raw operands (csrc/test_host.cpp; device pointers).
 * blocks int16 [n][64]: level-shifted samples (sample - 128), row-major 8x8; table uint8 [64]: a quantisation table
 * in natural order.  Per block the forward DCT, quantisation, dequantisation and IDCT of the round trip: coefs
 * int16 [n][64] the quantised coefficients (natural order), samples uint8 [n][64] the range-limited result,
 * outside int32 [n] 1 where the block left the exact range (what sets flags there; samples mean nothing then),
 * else 0.  Synchronous: the operands are read back and checked first.  MMF_EINVAL with nothing launched: a NULL
 * pointer, n outside 1..2^20, a misaligned pointer, a sample outside +-1024 (up to there 32-bit arithmetic is
 * exact; pixels give +-128), a zero table entry. */
int mmf_jpeg_block_roundtrip_raw(const int16_t* blocks, const uint8_t* table, int n, int16_t* coefs, uint8_t* samples,
                                 int32_t* outside, void* stream);

/* Test-only: mmf_resize_pil's plan for one width x height image (csrc/resize_host.cpp; host only, no handle, no
 * device call).  geom 0 = the EfficientNet squash (bilinear), 1 = CLIP's shortest edge -> 224 (bicubic) + centre
 * crop.  out12 int32 [12] (host) = ow, oh (Pillow's resize output size), cx, cy (the window's offset in it),
 * need_h, need_v (the pass runs: the size changes on that axis), y0, y1 (the source rows the horizontal pass
 * writes for the window's vertical taps), ksh, ksv (taps per coordinate; 1 for a pass that does not run), x0, x1
 * (0, 0, except where Image.resize runs the vertical pass first -- both passes run, height > 100 * width and the
 * height shrinks: then the source columns the vertical pass writes for the window's horizontal taps).
 * MMF_ERANGE: a pass needs more than 96 taps; MMF_EINVAL: a non-positive size, another geom, a NULL pointer.
 * mmf_resize_supported is 1 exactly where both geometries plan. */
int mmf_resize_plan(int width, int height, int geom, int32_t* out12);

/* Test-only: the coefficient kernel of mmf_resize_pil on that plan's one job (device pointers).  coef int32
 * [224 * ksh + 224 * ksv]: the 22-bit fixed-point weights of the 224 window coordinates, horizontal then vertical,
 * taps at and past a coordinate's n zero; bounds int32 [2][224][2]: (xmin, n) per axis (0 horizontal, 1 vertical)
 * and window coordinate.  An axis whose pass does not run has ks = 1 and values no pass reads.  Synchronous.
 * The same error codes, with nothing launched. */
int mmf_resize_coef_raw(int width, int height, int geom, int32_t* coef, int32_t* bounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HIP_H */
