/*
 * ccvpe_hip.h — C ABI of libccvpe_hip.so: the MI355X (gfx950) implementation of CCVPE's dense
 * cross-view matching forward path.
 *
 * The reference (tudelft-iv/CCVPE) has no FFI or plugin registry: the path sits behind a Python
 * nn.Module (`CVM_VIGOR.forward(grd, sat)`, /root/reference/models.py:150) that hands every
 * arithmetic step to a stock torch op.  Each entry point below therefore replaces one torch-op
 * group of that forward; the comment on each cites the reference lines it stands in for.  The
 * Python host (ccvpe_amd/models.py) binds them with ctypes — see INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller.
 *   - activations are fp32, NHWC ("pixel-major"): element (b,y,x,c) at ((b*H+y)*W+x)*ld + c with
 *     ld >= C the pixel stride in floats (lets a kernel write into a wider concat buffer).
 *   - the reference's NCHW fp32 tensors cross the boundary only at the two ends: the input images
 *     (stem kernel reads NCHW) and the returned heat-map / orientation / score tensors (written
 *     NCHW by the kernels that produce them).
 *   - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work on it (graph-capture
 *     safe: no allocation, no synchronisation, no host-side state).
 *   - return 0 on success, a negative CCVPE_E* code otherwise; ccvpe_last_error() gives the text.
 *     No C++ exception crosses the ABI.
 *   - devices and threads: a process may drive any number of devices.  A call launches on the HIP
 *     device that is current in the calling thread at call time (`stream` must belong to it).  What
 *     the library remembers about a device (a kernel's dynamic-LDS opt-in, the CU count) is kept per
 *     device ordinal in relaxed atomics: host threads may race on it, the worst case is a repeated
 *     driver call.  The error text and the host-side shape caches (row pitches, plane geometry) are
 *     per THREAD by design: ccvpe_last_error() reports the calling thread's last failure.
 */
#ifndef CCVPE_HIP_H
#define CCVPE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CCVPE_OK 0
#define CCVPE_EINVAL (-1)   /* bad argument (shape/alignment not supported) */
#define CCVPE_ELAUNCH (-2)  /* hipLaunchKernel / hipGetLastError failed     */

#define CCVPE_ACT_NONE 0
#define CCVPE_ACT_RELU 1
#define CCVPE_ACT_SWISH 2
#define CCVPE_ACT_RELU_MASK 3  /* out = residual > 0 ? value : 0 — the backward of a ReLU fused into the conv that produces its
                                 output gradient (residual = the ReLU's forward output; it is a mask here, not added) */

#define CCVPE_OUT_NHWC 0      /* dst[(pixel)*ldd + n]                                            */
#define CCVPE_OUT_DECONV2X 1  /* n = (dy*2+dx)*cout + co -> dst[(b,2y+dy,2x+dx)*ldd + co]        */

#define CCVPE_MAX_SHIFTS 48

const char* ccvpe_last_error(void);
int ccvpe_abi_version(void);

/* -------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on the fp32 matrix cores (v_mfma_f32_16x16x4_f32).
 *
 *   out[m, n] = act( (sum_{tap, c} in[pixel(m) + tap, c] * w[n, tap, c]) * scale[n] + shift[n] )
 *               (+ residual[m, n])
 *
 * One kernel covers every dense contraction of the path:
 *   1x1  : MBConv expand / project (+SE gate on the input, +skip) and the 320->1280 head
 *          (efficientnet_pytorch/model.py:62,86,104-106,121-130,209,299), the fused ground
 *          descriptor 1x1 convs (models.py:57-97)
 *   2x2/2: the aerial descriptor Linear over 2x2 patches (models.py:102-104,173-184)
 *   3x3  : double_conv, reading cat[deconv_out, skip] as two sources without materialising the
 *          concat (models.py:42-47,208-209,...)
 *   deconv: ConvTranspose2d(k=2,s=2) as one GEMM with N = 4*cout and a pixel-shuffle store
 *          (models.py:109-145)
 *
 * Weights are pre-packed by the host: w[n][k] row-major, k = tap*(c0+c1) + concat-channel,
 * K zero-padded to `kpad` (multiple of 16), N zero-padded to a multiple of 16 rows.
 * c0, c1 must be multiples of 8; ld0/ld1/ldd/ldres multiples of 4; pointers 16-byte aligned.
 * ----------------------------------------------------------------------------------------- */
typedef struct ccvpe_conv_desc {
  const float* src0; /* [B,H,W,ld0] first source                                   */
  const float* src1; /* [B,H,W,ld1] second (concatenated) source, or NULL           */
  const float* gate; /* [B,c0] per-sample per-channel multiplier on src0 (SE), NULL  */
  const float* w;    /* packed weights [npad16][kpad]                                */
  const float* scale;    /* [n] or NULL (=1)   folded BN scale                       */
  const float* shift;    /* [n] or NULL (=0)   folded BN shift / conv bias           */
  const float* residual; /* [M,ldres] or NULL  MBConv identity skip                  */
  float* dst;
  int c0, ld0, c1, ld1;
  int batch, in_h, in_w;
  int kh, kw, stride, pad; /* (1,1,1,0) (3,3,1,1) (2,2,2,0)                          */
  int n;                   /* real GEMM N (for deconv: 4*cout)                        */
  int kpad;
  int ldd, ldres;
  int act;      /* CCVPE_ACT_*  */
  int out_mode; /* CCVPE_OUT_*  */
} ccvpe_conv_desc;

int ccvpe_conv_igemm_f32(const ccvpe_conv_desc* desc, void* stream);

/* Split-K form for small-batch GEMMs (a handful of output tiles, thousands of K stages: decoder levels 6-5 and the late
 * encoder 1x1s at batch <= 8 leave most of the 256 CUs idle and walk K serially).  K is cut into slices, each slice
 * is its own workgroup row writing raw fp32 partial sums to `scratch`, and a second kernel adds the slices in index
 * order (deterministic) and applies the epilogue.  3x3 convs take the generic gather kernel in this mode.
 *   ccvpe_conv_igemm_splitk_floats: floats of scratch a split-K run of `desc` wants; 0 = splitting would not help
 *       (call ccvpe_conv_igemm_* instead); negative = error.
 *   ccvpe_conv_igemm_splitk_f32 / _bf16: same contract as ccvpe_conv_igemm_f32 / _bf16, with that scratch. */
int ccvpe_conv_igemm_splitk_floats(const ccvpe_conv_desc* desc, int is_bf16);
/* Which kernel the one-pass entry points (ccvpe_conv_igemm_f32 / _bf16) run for `desc`; launches nothing.  Returns
 * CCVPE_ROUTE_* | MT << 8 | NT << 12 | WN << 16 (workgroup tile = 16*MT*(4/WN) pixels x 16*NT*WN channels), or a negative
 * error code.  For tests ("did this shape reach the pointwise kernel?") and for bench.py's per-kernel accounting. */
#define CCVPE_ROUTE_IGEMM 0   /* generic gather kernel */
#define CCVPE_ROUTE_PW_GEMM 1 /* deep-stage pointwise kernel (1x1, stride 1, one source) */
#define CCVPE_ROUTE_CONV3X3 2 /* LDS-halo 3x3 kernel */
#define CCVPE_ROUTE_C3N 3     /* bf16 narrow 3x3 kernel: weights in registers, persistent workgroups (csrc/narrow_impl.h) */
#define CCVPE_ROUTE_PW_RING 4 /* pointwise kernel with a three-stage LDS-DMA ring, two workgroups per CU, fp32 and bf16 (csrc/conv_pw2_impl.h) */
#define CCVPE_ROUTE_PWN 5     /* (ABI 7) narrow projection kernel: N <= 48, K <= 256 (fp32: <= 144), weights x SE gate in registers, waves stream 16-pixel tiles (csrc/pwn.hip); the route's MT / NT fields hold N / 16 and K bytes / 64 */
int ccvpe_conv_igemm_route(const ccvpe_conv_desc* desc, int is_bf16, int out_f32);
/* Which form of the 3x3 kernel runs for a `desc` that routes to CCVPE_ROUTE_CONV3X3 (storage output, no out_f32):
 * NW | DMA << 4 | TPS << 8 — waves per workgroup (4 or 8: the 8-wave form doubles the pixel tile), W tile by LDS-DMA (1 for every
 * tile the kernel serves), taps per K stage (3 = a row of taps, 1).  0 for any other route, negative = error.  Host only: the
 * launcher's own decision (csrc/conv3x3_impl.h: conv3x3_variant), so that a test can assert the form before it launches. */
int ccvpe_conv3x3_variant(const ccvpe_conv_desc* desc, int is_bf16);
/* A/B switch for measurements (process-wide, default on): 0 sends the narrow bf16 decoder layers (CCVPE_ROUTE_C3N, and the
 * narrow form of ccvpe_upconv3x3_bf16) back to the tiled kernels.  Returns the previous setting. */
int ccvpe_set_narrow_kernels(int on);
/* The same kind of switch for CCVPE_ROUTE_PW_RING: 0 sends those fp32 pointwise layers back to CCVPE_ROUTE_PW_GEMM (bit-identical
 * results either way).  Returns the previous setting. */
int ccvpe_set_pw_ring_kernels(int on);
/* (ABI 7) The same kind of switch for CCVPE_ROUTE_PWN: 0 sends the narrow bf16 projections back to the generic kernel. */
int ccvpe_set_pwn_kernels(int on);
/* (ABI 7) The same kind of switch for the late-block MBConv front (csrc/mbconv_plane.hip: planes of <= 1024 pixels, Cin in
 * {80, 112, 192}), which runs behind the UNCHANGED ccvpe_mbconv_front_* / ccvpe_dwconv_* entry points and their *_nblk queries:
 * bit 0 = the fused expand + depthwise form (ccvpe_mbconv_front_nblk reports it), bit 1 = the depthwise-only form
 * (ccvpe_dwconv_*), bit 2 = the band-owner kernel for the fused form in bf16 storage (producer / consumer waves).  0 restores the round-5 chain (pointwise GEMM + dwconv_plane_kernel).  Returns the previous mode; change
 * it only between forwards (the *_nblk queries size the caller's squeeze-partial buffers). */
int ccvpe_set_mbconv_plane_kernels(int mode);
/* A 3x3 layer (desc: bf16 storage, one source, bias, no activation — convK.2 of double_conv, models.py:42-47) WITH the next
 * level's rotational matching in its epilogue, for ONE rotation hypothesis (the localisation branch of CVM_VIGOR_ori_prior(0):
 * models.py:489-500 with k = 0): replaces  x = convK.2(y);  scores, cat = match(x)  (models.py:211-228 pattern) — x never reaches
 * HBM.  desc->n = channels of x, desc->dst / ldd = the decoder input rows [x / max(|x|, 1e-12) | score | 0-pad] (ldd >= n + 1;
 * bf16, or fp32 with out_f32), scores [B,1,H,W] fp32; g [B][ldg] fp32 ground descriptor (first L entries), shift / stride /
 * window_offset as ccvpe_match_level.  Same formulas as ccvpe_match_level (no eps in the cosine).  _ok: 1 if the library serves
 * this layer / shape (narrow-level kernel, csrc/narrow_impl.h), else 0 — then run the two calls separately. */
/* fp32 3x3 layer (stride 1, pad 1, one source, bias only: convK.2 of double_conv, models.py:42-47) by Winograd F(2x2,3x3)
 * (csrc/conv3x3_wino.hip).  desc as for ccvpe_conv_igemm_f32 except `w`: the transformed weights U = G g G^T, packed
 * [round_up(n, 32)][16][round_up(c0, 16)] (row = output channel; component xi = 4 * row + column of the 4 x 4 grid, then
 * input channel; zero-padded), and kpad = 16 * round_up(c0, 16).  _ok: 1 if the kernel serves `desc` (H and W even,
 * c0 >= 32, batch * H * W >= 16384, not a shape the direct path splits along K), else 0 — then use ccvpe_conv_igemm_f32. */
int ccvpe_conv3x3_wino_ok(const ccvpe_conv_desc* desc);
int ccvpe_conv3x3_wino_f32(const ccvpe_conv_desc* desc, void* stream);
/* The same layer with all of its n <= 80 output channels in ONE workgroup (csrc/conv3x3_wino_n.hip): one input transform per tile
 * instead of one per 32 columns, 16-column granular matrix work; bit-identical to ccvpe_conv3x3_wino_f32.  desc and U pack as
 * above, 16 < n <= 80.  _ok: 0 = not served, 1 = computed correctly, 2 = also at or above the smallest launch at which
 * tools/wino_probe.py showed a win over ccvpe_conv3x3_wino_f32 (what models.py routes).  ccvpe_conv3x3_wino_match1_*: that kernel
 * with the next level's one-hypothesis matching in its epilogue — arguments and results exactly as ccvpe_conv3x3_match1_bf16
 * (below) in fp32 storage with the U pack as `w`; needs n % 4 == 0, ldd >= n + 1, 0 < L <= n.  ccvpe_set_wino_n(0) caps both
 * _ok values at 1 (A/B runs; the binding calls it for CCVPE_WINO_N=0); returns the previous setting. */
int ccvpe_conv3x3_wino_n_ok(const ccvpe_conv_desc* desc);
int ccvpe_conv3x3_wino_n_f32(const ccvpe_conv_desc* desc, void* stream);
int ccvpe_conv3x3_wino_match1_ok(const ccvpe_conv_desc* desc, int out_f32, int L);
int ccvpe_conv3x3_wino_match1_f32(const ccvpe_conv_desc* desc, int out_f32, const float* g, int ldg, int L, int shift, int stride,
                                  int window_offset, float* scores, void* stream);
int ccvpe_set_wino_n(int on);
int ccvpe_conv3x3_match1_ok(const ccvpe_conv_desc* desc, int out_f32, int L);
int ccvpe_conv3x3_match1_bf16(const ccvpe_conv_desc* desc, int out_f32, const float* g, int ldg, int L, int shift, int stride,
                              int window_offset, float* scores, void* stream);
int ccvpe_conv_igemm_splitk_f32(const ccvpe_conv_desc* desc, float* scratch, void* stream);

/* -------------------------------------------------------------------------------------------
 * ConvTranspose2d(k=2,s=2) folded into the 3x3 conv that follows it (models.py:207-209 and the same
 * pair at every decoder level of both branches: x = deconvK(x); x = cat[x, skip]; x = convK.0(x)).
 * Per output parity (py,px) the pair is one implicit GEMM over the LOW-RES pixels with 2x2 taps on
 * src0 and the ordinary 3x3 taps (stride 2, parity offset) on the skip:
 *   K = 4*c0 + 9*c1   instead of   9*(Cd + c1) + the deconv GEMM, and no upsampled intermediate.
 * w: [4][npad16][kpad] effective weights, parity-major ((py*2+px)), k = (du*2+dv)*c0 + ch for the
 * low-res source then 4*c0 + (ky*3+kx)*c1 + ch for the skip.  shift9: [9][n] = conv bias + the
 * deconv-bias terms of the 3x3 taps that fall inside the image, indexed by
 * (row class*3 + col class), class 0 = first row/col, 1 = interior, 2 = last.
 * ----------------------------------------------------------------------------------------- */
typedef struct ccvpe_upconv_desc {
  const void* src0;   /* [B,h1,w1,ld0] low-res input of the deconv (fp32 or bf16)   */
  const void* src1;   /* [B,2h1,2w1,ld1] skip, or NULL                              */
  const void* w;      /* packed effective weights                                    */
  const float* shift9;
  void* dst;          /* [B,2h1,2w1,ldd]                                             */
  int c0, ld0, c1, ld1;
  int batch, h1, w1;
  int n, kpad, ldd;
  int act;
} ccvpe_upconv_desc;

int ccvpe_upconv3x3_f32(const ccvpe_upconv_desc* desc, void* stream);
int ccvpe_upconv3x3_bf16(const ccvpe_upconv_desc* desc, void* stream);
/* Which kernel ccvpe_upconv3x3_f32 / _bf16 run for `desc`; launches nothing.  Returns CCVPE_UPROUTE_* | MT << 8 | NT << 12 |
 * WN << 16 (tile bits zero for CCVPE_UPROUTE_UP2), or a negative error code.  For tests and bench.py's per-kernel accounting. */
#define CCVPE_UPROUTE_GATHER 0   /* upconv_kernel: linear-M gather (low-res images narrower than 16 pixels) */
#define CCVPE_UPROUTE_HALO 1     /* upconv_halo_kernel: low-res halo in LDS, skip gathered, W through registers */
#define CCVPE_UPROUTE_DMA 2      /* upconv_dma_kernel (bf16): pair-of-taps stages, W by LDS-DMA */
#define CCVPE_UPROUTE_DMA_PAIR 3 /* upconv_dma_kernel, two 8 x 8 images per tile (level 6) */
#define CCVPE_UPROUTE_UP2 4      /* up2_kernel (bf16, narrow levels): four parities per workgroup, weights in registers */
int ccvpe_upconv3x3_route(const ccvpe_upconv_desc* desc, int is_bf16);
/* The same fp32 layer with its products on the bf16 matrix cores (csrc/upconv_s3.hip): every fp32 operand is split into three
 * bf16 planes (hi + mid + lo == the fp32 value exactly) and x.w is summed from six plane products in fp32 — fp32-class error,
 * not bit-identical to ccvpe_upconv3x3_f32.  desc as above (fp32 tensors, c1 > 0) except `w` / `kpad`: the three-plane pack
 * [4][stages][npad16][hi 16 | mid 16 | lo 16] bf16 in the kernel's stage order (models._pack_upconv_s3), stages =
 * 4*ceil(c0/16) + 9*ceil(c1/16), kpad = 48*stages.
 * ccvpe_upconv3x3_s3_ok launches nothing: 0 = not served (no skip, low-res images narrower than 16 pixels other than 8 x 8,
 * an n without a tile, a kpad that is not this pack's), 1 = computed correctly, 2 = and the measured size rule prefers it to
 * ccvpe_upconv3x3_f32.  ccvpe_upconv3x3_s3_f32 runs every desc with _ok >= 1 and returns CCVPE_EINVAL otherwise. */
int ccvpe_upconv3x3_s3_ok(const ccvpe_upconv_desc* desc);
int ccvpe_upconv3x3_s3_f32(const ccvpe_upconv_desc* desc, void* stream);
/* Two forms compute that layer: 1 = one output parity per workgroup (csrc/upconv_s3.hip, every served desc), 2 = "quad", all four
 * parities per workgroup (csrc/upconv_s3q.hip: 16 < n <= 80, images of 16 or more pixels a row; bit-identical to form 1 when
 * c1 <= 16).  ccvpe_upconv3x3_s3_f32 chooses by a measured size rule (form 0 = auto).
 * ccvpe_upconv3x3_s3_form_ok launches nothing: 0 = `form` cannot compute the desc, else the form that runs (for form 0: what
 * auto picks, 1 or 2).  ccvpe_upconv3x3_s3_form_f32 forces a form (0 = auto) and returns CCVPE_EINVAL for one that cannot serve
 * the desc.  ccvpe_set_s3_quad(0) makes auto never choose form 2 (A/B runs; the binding calls it for CCVPE_S3_QUAD=0); the
 * forcing entry point ignores it.  Returns the previous setting.
 * (ABI 7, additive) ccvpe_upconv3x3_s3_route launches nothing: the kernel ccvpe_upconv3x3_s3_form_f32(desc, form) would run, as
 * form that runs | pair << 4 | MT << 8 | NT << 12 | WN << 16 (pair: the two-images-per-tile kernel of 8 x 8 layers; the quad form:
 * MT = 2, NT = npad16 / 16, WN = 0), or 0 where _form_ok is 0.  For the launch recorder's names. */
int ccvpe_upconv3x3_s3_form_ok(const ccvpe_upconv_desc* desc, int form);
int ccvpe_upconv3x3_s3_route(const ccvpe_upconv_desc* desc, int form);
int ccvpe_upconv3x3_s3_form_f32(const ccvpe_upconv_desc* desc, int form, void* stream);
int ccvpe_set_s3_quad(int on);
/* (ABI 7, additive) The fp32 1x1 GEMMs behind the encoders' depthwise stage (MBConv project with the SE gate on its input, the
 * 320 -> 1280 head) and the two descriptor heads in the same three-plane arithmetic (csrc/pw_s3.hip): fp32-class error, not
 * bit-identical to ccvpe_conv_igemm_f32, bit-identical run to run (one pass, no K split).  desc as for ccvpe_conv_igemm_f32 —
 * fp32 tensors, one source, NHWC store, act none or swish, gate / scale / shift / residual as there — for (kh, kw, stride, pad) =
 * (1, 1, 1, 0) or (2, 2, 2, 0), c0 % 16 == 0, n > 48, except `w` / `kpad`: the three-plane pack [K / 16][npad16][hi 16 | mid 16 | lo 16]
 * bf16 (models._pack_pw_s3; k = (ky * 2 + kx) * c0 + channel as in the fp32 pack, stage = k / 16), kpad = 3 * K.
 * ccvpe_pw_s3_ok launches nothing: 0 = not served (any other layer, bf16 storage is the caller's to exclude, K % 16 != 0, a kpad
 * that is not this pack's, misaligned pointers), 1 = computed correctly, 2 = and the measured size rule prefers it to
 * ccvpe_conv_igemm_f32 (with its split-K second pass where it has one).  ccvpe_pw_s3_route launches nothing: 0 where _ok is 0, else
 * 1 | MT << 8 | NT << 12 | WN << 16 | NW << 20 of pw_s3_kernel<MT, NT, WN, NW> (NW waves; workgroup tile = 16*MT*(NW/WN) rows x
 * 16*NT*WN columns), for the launch recorder's names.  ccvpe_pw_s3_f32 runs every desc with _ok >= 1 and returns CCVPE_EINVAL otherwise.  What
 * ccvpe_conv_igemm_* route is unchanged. */
int ccvpe_pw_s3_ok(const ccvpe_conv_desc* desc);
int ccvpe_pw_s3_route(const ccvpe_conv_desc* desc);
int ccvpe_pw_s3_f32(const ccvpe_conv_desc* desc, void* stream);

/* -------------------------------------------------------------------------------------------
 * The whole 512 x 512 level of a decoder in one launch (csrc/tail512.hip):
 *   loc: x = deconv1(x); x = conv1(x)  [3x3 + ReLU + 3x3, 16 -> 16 -> 1]      models.py:124-127 (logits, :319)
 *   ori: x = deconv1_ori(x); x = conv1_ori(x) [16 -> 16 -> 2]; F.normalize    models.py:145-148,341
 * x [B,h1,w1,ld0] low-res input (c0 channels incl. zero padding; fp32 or bf16), w / shift9 as for ccvpe_upconv3x3
 * with n = 16 and c1 = 0 ([4][16][kpad], [9][16]), w2 [cout][3][3][16] fp32, b2 [cout], out [B,cout,2h1,2w1] fp32
 * (NCHW).  The 16-channel intermediate is never written.  h1, w1 multiples of 16.  Same results as ccvpe_upconv3x3 +
 * ccvpe_head_conv3x3 (fp32: to rounding; bf16: better — the intermediate is not rounded to bf16).
 * split (ccvpe_tail512_f32 only): 0 = exact fp32 matrix arithmetic; 1 (cout = 1 only) = the fp32 operands are split into bf16 hi + lo
 * planes and multiplied on the bf16 matrix cores (hi.hi + lo.hi + hi.lo, fp32 accumulate: ~1e-5 of scale instead of bit-level
 * fp32) — the fp32 tail of the bf16 STORAGE path (set_precision("bf16")), never used by the fp32 path; 2 (cout = 1 with up to 48
 * channels AND cout = 2 with up to 32) = three bf16 planes per operand, hi + mid + lo == the fp32 value, x.w summed from the six
 * products hh, hm, mh, mm, hl, lh in fp32 (the convention of ccvpe_upconv3x3_s3_f32; W is split inside the kernel from the same
 * fp32 pack) — fp32-class error, not bit-identical to split = 0; the fp32 path's tails.  Any other value, and any (split, cout,
 * c0) the library has no kernel for, is refused with CCVPE_EINVAL before anything is launched.
 * ----------------------------------------------------------------------------------------- */
typedef struct ccvpe_tail_desc {
  const void* x;
  const void* w;
  const float* shift9;
  const float* w2;
  const float* b2;
  float* out;
  int batch, h1, w1;
  int c0, ld0, kpad;
  int cout, normalize, split;
  float* softmax_partial;   /* cout = 1, optional (NULL: not written): [B][ccvpe_tail512_partials()][2] = (max, sum exp(l - max)) of the
                               logits of every (tile, wave) — the heat-map softmax (models.py:319-320) then needs no row-wide max /
                               sum sweep: ccvpe_softmax_apply_f32 */
} ccvpe_tail_desc;

int ccvpe_tail512_f32(const ccvpe_tail_desc* desc, void* stream);
int ccvpe_tail512_bf16(const ccvpe_tail_desc* desc, void* stream);
int ccvpe_tail512_partials(const ccvpe_tail_desc* desc, int is_bf16);   /* partial pairs per sample for this descriptor (launches nothing) */
/* Softmax(dim=-1) over rows of n logits from n_partials (max, sum exp) pairs per row (models.py:320): out = exp(l - M) / S. */
int ccvpe_softmax_apply_f32(const float* logits, const float* partials, int n_partials, float* out, int rows, int n,
                            void* stream);

/* -------------------------------------------------------------------------------------------
 * The WHOLE eval forward behind one entry point (csrc/plan.hip) — replaces the call sites
 *   logits, heatmap, ori, score1..6 = model(grd, sat)      train_VIGOR.py:252-254,282 / train_KITTI.py:285-287,302 /
 *                                                           visualize_qualitative_results_VIGOR.py:68-71
 * for a model in eval mode (models.py:150-343, :448-652, :752-950, :954-1246).
 * A ctx is created from a PLAN: the launch list of one forward for fixed (model, weights, batch, image sizes, precision),
 * recorded and serialised by ccvpe_amd/plan.py (or read from a file the Python side wrote: tools/plan_run.cpp is a caller
 * without Python).  plan: the serialised bytes (header, calls, descriptor blobs, packed weights).
 * weights_dev / workspace_dev: device buffers of at least the plan's weights / workspace size (ccvpe_ctx_info on a ctx, or the
 * Python Plan object) owned by the CALLER — or NULL: the library allocates and frees them.  The weights are uploaded here.
 * ccvpe_forward: grd [B,3,h,w], sat [B,3,H,W] NCHW fp32 device tensors of the recorded shapes; every kernel is enqueued on
 * `stream` (capturable in a hipGraph); out (may be NULL) receives the device pointers of the nine outputs — fp32, NCHW-
 * contiguous, inside the ctx's workspace, valid until the next ccvpe_forward on this ctx.  One ctx serves one stream at a time.
 * Errors: int status, ccvpe_last_error() names the failing call.
 * ----------------------------------------------------------------------------------------- */
typedef struct ccvpe_ctx ccvpe_ctx;
int ccvpe_ctx_create(const void* plan, long long n_bytes, void* weights_dev, void* workspace_dev, ccvpe_ctx** ctx);
int ccvpe_ctx_destroy(ccvpe_ctx* ctx);
int ccvpe_ctx_info(const ccvpe_ctx* ctx, long long* workspace_bytes, long long* weights_bytes, long long* grd_bytes,
                   long long* sat_bytes, int* n_outputs, int* n_calls);
int ccvpe_ctx_output(const ccvpe_ctx* ctx, int i, void** dev_ptr, long long* bytes, int* ndim, long long* dims4,
                     long long* strides4);   /* strides in ELEMENTS: an output may be a view (ori_prior's score1 is a channel slice) */
int ccvpe_forward(ccvpe_ctx* ctx, const void* grd, const void* sat, void** out, void* stream);

/* -------------------------------------------------------------------------------------------
 * EfficientNet stem: 3x3 stride-2 conv on the NCHW image + folded BN + swish, NHWC out.
 * TF-"SAME" padding (0 before, 1 after) from the 224 schedule; `circular` wraps along W and
 * zero-pads along H.  efficientnet_pytorch/model.py:181-182,289; utils.py:254-282,318-358.
 *   x [B,3,H,W] NCHW, w [3][3][3][32] (ky,kx,ci,co), y [B,H/2,W/2,32]
 * ----------------------------------------------------------------------------------------- */
int ccvpe_stem_conv_f32(const float* x_nchw, const float* w, const float* scale, const float* shift,
                        float* y, int batch, int in_h, int in_w, int circular, void* stream);

/* -------------------------------------------------------------------------------------------
 * Depthwise kxk conv (k in {3,5}, stride in {1,2}) + folded BN + swish, and the squeeze half of
 * squeeze-excite: per-(sample, channel) partial sums of the activated output, one row per
 * workgroup (fixed order => deterministic), reduced later by ccvpe_se_gate_f32.
 * efficientnet_pytorch/model.py:70-73,108-110,114; padding as for the stem
 * (stride 1: (k-1)/2 both sides; stride 2: k=3 (0,1), k=5 (1,2)).
 *   x [B,H,W,C] (ld=C), w [k][k][C], y [B,Ho,Wo,C], se_partial [B][nblk][C]
 * ccvpe_dwconv_nblk() returns nblk for a given shape (so the caller can size se_partial).
 * ----------------------------------------------------------------------------------------- */
int ccvpe_dwconv_nblk(int in_h, int in_w, int channels, int stride);
int ccvpe_dwconv_f32(const float* x, const float* w, const float* scale, const float* shift, float* y,
                     float* se_partial, int batch, int in_h, int in_w, int channels, int k, int stride,
                     int circular, void* stream);

/* -------------------------------------------------------------------------------------------
 * Stem + MBConv block 0 front half in one launch (eval): ccvpe_stem_conv + ccvpe_dwconv(k = 3, stride 1, 32
 * channels) + the SE squeeze partials, with the [B, H/2, W/2, 32] stem tensor kept in LDS
 * (efficientnet_pytorch/model.py:289 then :108-110,114 of block 0, which has no expand conv).  fp32: the
 * same bits as the two unfused calls.
 * ccvpe_stem_dw_nblk() returns the number of SE partial rows per sample (8 x 32 output tiles), 0 if the shape
 * is not supported (circular padding with an odd width): then use the two unfused calls.
 *   x_nchw [B,3,H,W] fp32, w [27][32], w_dw [3][3][32], y [B,Ho,Wo,32], se_partial [B][nblk][32]
 * ----------------------------------------------------------------------------------------- */
int ccvpe_stem_dw_nblk(int in_h, int in_w, int circular);
int ccvpe_stem_dw_f32(const float* x_nchw, const float* w, const float* s0, const float* b0, const float* w_dw,
                      const float* s1, const float* b1, float* y, float* se_partial, int batch, int in_h,
                      int in_w, int circular, void* stream);
int ccvpe_stem_dw_bf16(const float* x_nchw, const float* w, const float* s0, const float* b0, const float* w_dw,
                       const float* s1, const float* b1, void* y, float* se_partial, int batch, int in_h,
                       int in_w, int circular, void* stream);

/* -------------------------------------------------------------------------------------------
 * Fused MBConv front half for the early (large) blocks: expand 1x1 + BN0 + swish -> depthwise kxk +
 * BN1 + swish + SE squeeze partials, with the 6x-expanded tensor kept in LDS
 * (efficientnet_pytorch/model.py:102-110,114).  Same results as ccvpe_conv_igemm_f32 followed by
 * ccvpe_dwconv_f32.  w_exp is the igemm-packed expand weight [mid^16][kpad].
 * ccvpe_mbconv_front_nblk() returns the number of SE partial rows per sample, 0 if the shape is
 * not supported (then use the two unfused calls), <0 on bad arguments.
 *   x [B,H,W,cin], y [B,Ho,Wo,mid], se_partial [B][nblk][mid]
 * ----------------------------------------------------------------------------------------- */
int ccvpe_mbconv_front_nblk(int in_h, int in_w, int cin, int mid, int k, int stride);
/* (ABI 7) which kernel the fused call runs for a shape — 0 none (use the unfused calls), 1 mbconv_front_kernel (early blocks),
 * 2 mbconv_plane_kernel, 3 mbconv_band_kernel (late blocks: planes of <= 1024 pixels; 3 = bf16 storage only).  Reporting only. */
int ccvpe_mbconv_front_route(int in_h, int in_w, int cin, int mid, int k, int stride, int is_bf16, int batch);
/* The mbconv_band_kernel<k, stride, nkk, tpw, ry> instantiation and the chunk grouping that ccvpe_mbconv_front_bf16 launches
 * for a shape: nkk | tpw << 4 | ry << 8 | cpg << 12 | ngrp << 20 (nkk = 32-channel K pieces of the expand conv, tpw = the
 * 10- or 4-tile class, ry = output rows per depthwise thread, cpg = 16-channel slices per workgroup, ngrp = workgroups per
 * sample and band; cpg depends on the device's CU count and on batch), or 0 when route != 3.  Host only; the launcher,
 * ccvpe_mbconv_front_route and this query share one helper (csrc/mbconv_plane.hip: mbband_plan). */
int ccvpe_mbconv_band_plan(int in_h, int in_w, int cin, int mid, int k, int stride, int batch);
int ccvpe_mbconv_front_f32(const float* x, const float* w_exp, int kpad, const float* s0, const float* b0,
                           const float* w_dw, const float* s1, const float* b1, float* y, float* se_partial,
                           int batch, int in_h, int in_w, int cin, int mid, int k, int stride, int circular,
                           void* stream);
/* (ABI 7, additive) The fp32 early blocks with the expand 1x1 on the bf16 matrix cores in the three-plane arithmetic of
 * ccvpe_upconv3x3_s3_f32 / ccvpe_pw_s3_f32 (csrc/mbconv_front.hip: mbconv_front_s3_kernel): fp32-class error, not bit-identical to
 * ccvpe_mbconv_front_f32, bit-identical run to run.  Arguments as ccvpe_mbconv_front_f32 except `w_exp3` / `kpad`: the three-plane
 * pack [ceil(cin / 16)][mid][hi 16 | mid 16 | lo 16] bf16 of the fp32 pack (models._pack_pw_s3), kpad = 48 * ceil(cin / 16).  Tile
 * geometry and se_partial rows are those of ccvpe_mbconv_front_nblk.  Served: EfficientNet-B0's blocks 1-5, (k, stride, cin) =
 * (3, 2, <= 16), (3, 1, 17..32), (5, 2, 17..32), (5, 1, 33..48), (3, 2, 33..48).  ccvpe_mbconv_front_s3_ok launches nothing: 0 = not
 * served (bf16 storage is the caller's to exclude), 1 = computed correctly, 2 = and the measured size rule prefers it to
 * ccvpe_mbconv_front_f32.  ccvpe_mbconv_front_s3_f32 runs every shape with _ok >= 1 and returns CCVPE_EINVAL otherwise. */
int ccvpe_mbconv_front_s3_ok(int in_h, int in_w, int cin, int mid, int k, int stride, int batch);
int ccvpe_mbconv_front_s3_f32(const float* x, const void* w_exp3, int kpad, const float* s0, const float* b0,
                              const float* w_dw, const float* s1, const float* b1, float* y, float* se_partial,
                              int batch, int in_h, int in_w, int cin, int mid, int k, int stride, int circular,
                              void* stream);

/* Squeeze-excite gate: mean -> 1x1 (C->Cs) + swish -> 1x1 (Cs->C) -> sigmoid.
 * efficientnet_pytorch/model.py:113-118.  w1 [Cs][C], w2 TRANSPOSED [Cs][C], gate [B][C]. */
int ccvpe_se_gate_f32(const float* se_partial, int nblk, float inv_hw, const float* w1, const float* b1,
                      const float* w2, const float* b2, float* gate, int batch, int channels,
                      int squeezed, void* stream);

/* -------------------------------------------------------------------------------------------
 * Ground descriptors: height collapse of the fused 1x1-conv output.
 *   D_l[b, x*Cd_l + c] = sum_y wh_l[y] * y1[b,y,x,off_l + c] + bh_l      (models.py:57-97)
 * y1 [B,h,w,ld] holds all six heads' channels side by side (conv bias already added);
 * out [B][sum_l w*Cd_l], level l at offset w*off_l.  wh [6][h], bh [6], cd [6].
 * ----------------------------------------------------------------------------------------- */
int ccvpe_ground_descriptor_f32(const float* y1, int ld, const float* wh, const float* bh, const int* cd,
                                float* out, int batch, int h, int w, void* stream);

/* (ABI 7) A/B switch of the matrix-core form of ccvpe_match_level_* (9 <= n_shifts <= 32, even table offsets: the circulant
 * [n_shifts x C] of the ground descriptor times the [C x pixels] tile as v_mfma_f32_16x16x4_f32, exact fp32).  0 = the vector-ALU
 * form for every configuration, 1 = the tiled matrix-core form, 2 (default) = additionally the streaming form of the narrow levels
 * (C <= 80, no tail scores, >= 65 536 pixels: every wave streams 16-pixel tiles, no LDS).  Returns the previous setting. */
int ccvpe_set_match_mfma(int on);
/* Which kernel form ccvpe_match_level_f32 (elem_size 4) / _bf16 (elem_size 2) launches for these arguments, decided by the same
 * host function as the launch and without touching the device: returns 0 = vector-ALU form, 1 = tiled matrix-core form,
 * 2 = streaming form (it honours ccvpe_set_match_mfma), or the negative error code the launch would return (the pointer
 * alignment and ldg checks excepted: the query takes neither).  out (may be NULL) receives CCVPE_MATCH_ROUTE_INTS ints, 0 where a
 * field does not apply to the form: [0] NPAD, the hypothesis rows of the instantiation (16 MTL for the streaming form),
 * [1] PARTIAL (L < channels), [2] VEC, the widest aligned read of the descriptor table (tiled forms), [3] NB, the 16-channel
 * blocks of the streaming form, [4] LPP lanes per pixel and [5] TP pixels per workgroup (tiled forms), [6] NPT 16-pixel tiles
 * and [7] KS K slices per tile (matrix-core form), [8] the LDS row pitch S in floats and [9] the dynamic LDS bytes (tiled
 * forms).  The streaming form's tiles per wave depend on the device's CU count and are not reported. */
#define CCVPE_MATCH_ROUTE_INTS 10
int ccvpe_match_route(int elem_size, int L, const int* shifts, int n_shifts, int n_max, int n_tail, int stride,
                      int window_offset, int ldx, int ldo, int batch, int hw, int channels, int* out);
/* -------------------------------------------------------------------------------------------
 * Rotational matching + LMU concat, fused (models.py:186-205 and the five blocks after it;
 * ori_prior :484-514; KITTI :788-806):
 *   score[b,i,p] = sum_{c<L} g[b,c] * X[b,p,(c + shift_i*stride) mod C]
 *                  / ( ||X[b,p,window_i]||_2 * ||g[b]||_2 )               (no eps, as upstream)
 *   dstx[b,p,0:C]        = X[b,p,:] / max(||X[b,p,:]||_2, 1e-12)
 *   dstx[b,p,C]          = max_{i < n_max} score[b,i,p]
 *   dstx[b,p,C+1+j]      = score[b, n_max_first + j, p]   j < n_tail   (level-1 orientation input)
 *   dstx[b,p,C+1+n_tail : ldo] = 0
 * X [B,H*W,ldx]; g [B,ldg] (first L entries); scores [B,n_shifts,H*W] (NCHW, returned to caller).
 * The first n_max shifts feed the max; the last n_tail shifts are also copied into dstx.
 * window_offset: first channel of the L-wide window inside the rolled volume — 0 for VIGOR / KITTI, int(C/2 - L/2)
 * for CVM_OxfordRobotCar's centred window (models.py:1094): window_i[c] = X[(c + window_offset + shift_i*stride) mod C].
 * ----------------------------------------------------------------------------------------- */
int ccvpe_match_level_f32(const float* x, int ldx, const float* g, int ldg, int L, const int* shifts,
                          int n_shifts, int n_max, int n_tail, int stride, int window_offset, float* scores,
                          float* dstx, int ldo, int batch, int hw, int channels, void* stream);

/* -------------------------------------------------------------------------------------------
 * Final 3x3 conv to 1 or 2 channels, NCHW out (models.py:125-127 conv1.2, :146-148 conv1_ori.2);
 * normalize!=0 divides the 2-vector by max(norm,1e-12) (models.py:341).
 * x [B,H,W,16] NHWC, w [cout][3][3][16], out [B,cout,H,W].
 * ----------------------------------------------------------------------------------------- */
int ccvpe_head_conv3x3_f32(const float* x, const float* w, const float* bias, float* out_nchw, int batch,
                           int h, int w_, int cout, int normalize, void* stream);

/* Row softmax over n columns (models.py:319-320: Softmax over the 262144 flattened logits). */
int ccvpe_softmax_rows_f32(const float* logits, float* out, int rows, int n, void* stream);
/* bf16 -> fp32 widening of an activation tensor (n_elems % 8 == 0, 16-byte aligned): the bf16 storage path runs its last
 * localisation-decoder levels through the fp32 kernels (models.py:299-320 decide the heat-map arg-max). */
/* n device-to-device copies of fp32 vectors (counts[i] floats from srcs[i] to dsts[i]) in ceil(n / 96) launches; the three
 * arrays are HOST arrays, read before the call returns.  Gradients -> slots of the flat all-reduce arena (harness.py). */
int ccvpe_multi_copy_f32(const void* const* srcs, void* const* dsts, const int* counts, int n, void* stream);
/* Train-mode weight re-pack in ONE launch (train_VIGOR.py:146-150: optimizer.step() rewrites every weight, so every step
 * re-lays all of them out for the forward and backward GEMMs).  n_chunks chunks; chunk c writes counts[c] (<=
 * ccvpe_gather_repack_chunk()) floats to dsts[c]: element i = idx[idx_off[c] + i] > 0 ? srcs[c][idx[idx_off[c] + i] - 1] : 0.
 * All five arrays are DEVICE arrays (built once per parameter placement by ccvpe_amd/repack.py). */
int ccvpe_gather_repack_f32(void* const* dsts, const void* const* srcs, const long long* idx_off, const int* counts,
                            const int* idx, int n_chunks, void* stream);
int ccvpe_gather_repack_chunk(void);
int ccvpe_cast_bf16_f32(const void* src, float* dst, long n_elems, void* stream);

/* -------------------------------------------------------------------------------------------
 * Evaluation post-processing on the device (train_VIGOR.py:294-324, train_KITTI.py:304-343): per
 * sample the arg-max pixel of the heat-map (first maximum, as numpy.argmax), the orientation
 * vector there and the acos-based angle in degrees — 6 floats per sample instead of a 3 MB D2H
 * copy of the full maps:   out[b] = { y, x, cos, sin, angle_deg (NaN if |cos|>1 or |sin|>1), prob }.
 *   heatmap [B,h*w], ori [B,2,h*w] (NCHW), out [B,6]
 * ----------------------------------------------------------------------------------------- */
int ccvpe_eval_postprocess_f32(const float* heatmap, const float* ori, float* out, int batch, int h, int w,
                               void* stream);

/* -------------------------------------------------------------------------------------------
 * The reference test protocols' whole per-sample loop body in one launch (train_KITTI.py:304-343,
 * train_OxfordRobotCar.py:218-246, train_VIGOR.py:294-326): first-maximum arg-max of the heat-map AND of
 * the ground-truth map (ties to the smallest index, as numpy.argmax), then in double precision
 *   rows[b] = { pred_y, pred_x, gt_y, gt_x,
 *               pixel distance, metres (= distance * metres_per_pixel[b]),
 *               longitudinal metres = |cos(angle_diff * pi / 180) * distance| * metres_per_pixel[b],
 *               lateral metres      = |sin(angle_diff * pi / 180) * distance| * metres_per_pixel[b],
 *               predicted angle in degrees (NaN if |cos| > 1 or |sin| > 1 at the arg-max, compared in float),
 *               orientation error min(|d|, 360 - |d|) against the angle of gt_ori at the GT arg-max (NaN likewise),
 *               heatmap[pred], heatmap[gt] }
 * with angle_diff = |heading_deg[b] - atan2(|gt_x - pred_x|, |gt_y - pred_y|) * 180 / pi|; heading_deg is used as
 * given (no wrap).  heatmap, gt [B,h*w]; ori, gt_ori [B,2,h*w] (NCHW); heading_deg, metres_per_pixel [B] doubles;
 * rows [B,12] doubles, 8-byte aligned — any row of a larger table.  16-byte loads when h*w % 4 == 0 and both maps
 * are 16-byte aligned, scalar loads otherwise.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_eval_metrics_f32(const float* heatmap, const float* ori, const float* gt, const float* gt_ori,
                           const double* heading_deg, const double* metres_per_pixel, double* rows, int batch, int h,
                           int w, void* stream);

/* -------------------------------------------------------------------------------------------
 * Sequence localisation: one step of a histogram filter over the heat-map grid, per track b (ccvpe_amd.tracking.step_spec
 * is the specification, in numpy float64).  Two launches, no host read-back, no allocation, no floating-point atomics
 * (two runs are bit-identical):
 *   predict  Q[y,x] = sum_i ky[i+R] sum_j kx[j+R] prior[y - oy - i, x - ox - j], prior = 0 outside the grid (mass that
 *            leaves the grid is lost; a one-hot prior at (y0,x0) with R = 0 and offset (3,-5) gives Q one-hot at (y0+3, x0-5));
 *            the row pass, then the column pass, in fp32
 *   measure  M = (1 - outlier) heat + outlier / (h w);  U = Q M;  Z = sum U, S = sum Q (double)
 *   reset    1 when reset[b] != 0 (the predict is skipped, S = 0), 2 when not (Z > 0 and finite): U := M, Z := sum M
 *   post     = U (float)(1 / Z)
 *   rows[b]  = { pred_y, pred_x (first maximum of U, ties to the smallest index, NaN skipped), post there, cos, sin (ori
 *                there), angle in degrees (ccvpe_eval_metrics_f32's rule; NaN if |cos| > 1 or |sin| > 1 in float), Z,
 *                reset (0, 1, 2), mean_y, mean_x, var_yy, var_xx, cov_yx of U / Z over integer pixel coordinates, S }
 * prior, heat, post [B,h*w] (post must not overlap prior, heat or ori; the prior of a reset track is not read); ori [B,2,h*w];
 * offsets [B,2] (oy, ox), any int32; taps [B,2,2R+1] (y then x), >= 0; 0 <= radius <= 32; 0 <= outlier <= 1; reset [B] or
 * NULL; scratch: batch * ccvpe_belief_partials(h, w) doubles (ccvpe_belief_partials launches nothing; CCVPE_EINVAL for a
 * bad shape); rows [B,14] doubles — any rows of a larger table; rows and scratch 8-byte aligned.  16-byte loads of the prior
 * when w % 4 == 0 and it is 16-byte aligned, of heat / post when h*w % 4 == 0 and they are.  Non-finite inputs: the call
 * returns, reset is 2 and the rest of the row is unspecified.
 *
 * ccvpe_belief_step_rigid_f32 (specification: tracking.step_rigid_spec): the same step with the predict replaced by a rigid
 * motion of the grid — a warp, then the same blur.  motion [B,6] doubles (a00, a01, a02, a10, a11, a12), the INVERSE map
 * (tracking.rigid_motion), 8-byte aligned, any values:
 *   warp     W[y,x] = bilinear sample of the prior (0 outside the grid) at sy = (a00 y + a01 x) + a02, sx = (a10 y + a11 x)
 *            + a12, each product and sum rounded to double in that order; y0 = floor(sy), weights (float)(sy - y0) and
 *            (float)(1 - (sy - y0)), likewise in x; top = wx0 v00 + wx1 v01, bot = wx0 v10 + wx1 v11, W = wy0 top + wy1 bot
 *            in fp32 (a product, then one fma); 0 where (sy, sx) is not finite or not in (-1, h) x (-1, w)
 *   predict  Q = the separable blur of W with taps (centred taps: sub-pixel shifts live in the warp); W is taken on the grid
 *            plus the blur's halo, not cropped before the blur
 * Every other argument, the scratch size, the rows and the reset rules are those of ccvpe_belief_step_f32; for a00 = a11 = 1,
 * a01 = a10 = 0 and integer a02 = -oy, a12 = -ox the two give the same bits.  Same launches: two, no floating-point atomics.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_belief_partials(int h, int w);
int ccvpe_belief_step_f32(const float* prior, const float* heat, const float* ori, const int* offsets, const float* taps,
                          int radius, float outlier, const int* reset, float* post, double* scratch, double* rows,
                          int batch, int h, int w, void* stream);
int ccvpe_belief_step_rigid_f32(const float* prior, const float* heat, const float* ori, const double* motion,
                                const float* taps, int radius, float outlier, const int* reset, float* post, double* scratch,
                                double* rows, int batch, int h, int w, void* stream);

/* -------------------------------------------------------------------------------------------
 * The backward step of the forward-backward smoother over the same grid, per track b, for the pair of frames (s, t = s + 1)
 * (ccvpe_amd.tracking.smooth_step_spec / smooth_step_rigid_spec are the specifications).  Two launches, no read-back, no
 * allocation, no floating-point atomics (two runs are bit-identical):
 *   measure       M = (1 - outlier) heat + outlier / (h w) as the forward step rounds it;  G = M beta
 *   back-predict  B'[y,x] = sum_i ky[i+R] sum_j kx[j+R] G[y + oy + i, x + ox + j], G = 0 outside the grid: the exact adjoint of
 *                 the forward predict.  offsets and taps are the FORWARD step's own (of frame t); the sign and the reversal of
 *                 the taps live in the kernel's index arithmetic
 *   outputs       V = alpha B', Z = sum V, S = sum B' (double);  smooth = V (float)(1 / Z);  beta_out = B' (float)(1 / S)
 *   state         0; 1 when cut[b] != 0 (frame s is the last of its segment: the back-predict is skipped, S = 0); 2 when not
 *                 (Z > 0 and finite and S > 0 and finite).  In states 1 and 2 smooth = alpha (float)(1 / sum alpha),
 *                 Z = sum alpha and every pixel of beta_out is (float)(1 / (h w))
 *   rows[b]       the forward step's 14 columns: first maximum of V (of alpha in states 1, 2), smooth there, ori there and its
 *                 angle, Z, the state, mean and covariance of smooth, S
 * beta: the backward message of frame t, any positive scale; heat: the heat-map of frame t; alpha: the filter's posterior of
 * frame s; ori [B,2,h*w] of frame s; cut [B] or NULL.  beta_out and smooth [B,h*w] must not overlap each other or beta, heat,
 * alpha, ori.  scratch, rows, alignment, radius and outlier as ccvpe_belief_step_f32.
 *
 * ccvpe_belief_smooth_step_rigid_f32: motion [B,6] doubles, the FORWARD rigid step's own rows (of frame t), 8-byte aligned.
 * The kernel inverts each row (the general 2 x 2 inverse in double, every operation rounded on its own, as
 * tracking.invert_motion; NaN rows, which sample nothing, for a singular or non-finite row) and takes
 *   B' = blur(warp(G; inverted row), taps reversed)    with ccvpe_belief_step_rigid_f32's warp rule.
 * This is NOT the exact adjoint of the rigid predict (the adjoint of a bilinear gather is a scatter): it is the same continuous
 * model discretised along the reverse motion — exact in the continuum because the blur is isotropic and the motion has unit
 * Jacobian.  For angle 0 or quarter turns with whole-pixel shifts it gives the translate form's values.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_belief_smooth_step_f32(const float* beta, const float* heat, const float* alpha, const float* ori, const int* offsets,
                                 const float* taps, int radius, float outlier, const int* cut, float* beta_out, float* smooth,
                                 double* scratch, double* rows, int batch, int h, int w, void* stream);
int ccvpe_belief_smooth_step_rigid_f32(const float* beta, const float* heat, const float* alpha, const float* ori,
                                       const double* motion, const float* taps, int radius, float outlier, const int* cut,
                                       float* beta_out, float* smooth, double* scratch, double* rows, int batch, int h, int w,
                                       void* stream);

/* -------------------------------------------------------------------------------------------
 * The most likely path over the grid (max-product / Viterbi; specification: tracking.viterbi_step_spec and
 * tracking.backtrack_spec).  No back-pointer maps: the decision of a link is recomputed at the one pixel the path visits.
 *
 * ccvpe_belief_viterbi_step_f32: ccvpe_belief_step_f32 with the sums of the predict replaced by maxima,
 *   P[y,x] = max(0, max_i ky[i+R] * max(0, max_j kx[j+R] * prior[y - oy - i, x - ox - j])),   U = P M,  post = U (float)(1 / Z)
 * every product rounded once to fp32, NaN products ignored (fmaxf).  The map is normalised by its SUM (launch two is the
 * filter's own), so its peak stays at or above 1 / (h w).  Arguments, checks, scratch, rows and reset rules: those of
 * ccvpe_belief_step_f32; rows[b][13] holds sum P.  Two launches, no atomics.
 *
 * ccvpe_belief_backtrack_f32: ONE launch for a whole drive, one workgroup per track.  deltas [T,B,h*w]: the posts of the
 * forward pass; ori [T,B,2,h*w]; offsets [T,B,2] and taps [T,B,2,2R+1]: the motion INTO each frame; rows [T,B,14]: the forward
 * rows; reset [T,B] or NULL (frame 0 always starts a segment); path [T,B,8] doubles out:
 *   { y, x, deltas there, cos, sin, angle, link, score }
 * Frame T-1 takes its row's arg-max (link 1).  For t >= 1: if reset[t] != 0 or rows[t][7] != 0, frame t-1 takes its row's
 * arg-max (link 1); else the candidates are the source pixels (y_t - oy - i, x_t - ox - j), |i|, |j| <= R, inside the grid,
 * with value ky[i+R] * (kx[j+R] * deltas[t-1]) (fp32, each product rounded once — the bits of P there); only positive finite
 * values compete; the largest wins, the smaller flat index on equal values (link 0, score = the value); with no candidate
 * frame t-1 takes its row's arg-max (link 2, score 0).  Pixels read from rows are clamped to the grid.  path must not
 * overlap an input; rows and path 8-byte aligned; 0 <= radius <= 32.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_belief_viterbi_step_f32(const float* prior, const float* heat, const float* ori, const int* offsets, const float* taps,
                                  int radius, float outlier, const int* reset, float* post, double* scratch, double* rows,
                                  int batch, int h, int w, void* stream);
int ccvpe_belief_backtrack_f32(const float* deltas, const float* ori, const int* offsets, const float* taps, int radius,
                               const double* rows, const int* reset /* may be null */, double* path, int frames, int batch, int h,
                               int w, void* stream);

/* -------------------------------------------------------------------------------------------
 * Losses (losses.py:4-29), device scalars out.  `acc` is caller-provided scratch.
 *   infoNCE: accumulates num = sum_{label>1e-2} log(softmax(s/T))*label and den = sum label over
 *            the whole batch; loss = -num/den.            scores/labels [B,n]
 *            ONE pass over the data with (chunk, sample) workgroups.  rows [4*B + 4] floats out: per sample
 *            (num_b, den_b, z_b = sum exp(s/T), 0), then the batch label mass — the backward reads them instead of
 *            recomputing row statistics.  scratch: ccvpe_infonce_scratch_floats(batch, n) floats.
 *   CE     : -sum(labels*log_softmax(logits))/B           [B,n]
 *   ori    : sum(||gt_ori-ori||^2 * gt)/B                 ori/gt_ori [B,2,hw], gt [B,hw]
 * ----------------------------------------------------------------------------------------- */
int ccvpe_infonce_scratch_floats(int batch, int n);
int ccvpe_infonce_loss_f32(const float* scores, const float* labels, float temperature, float* loss,
                           float* rows, float* scratch, int batch, int n, void* stream);
int ccvpe_cross_entropy_loss_f32(const float* logits, const float* labels, float* loss, float* scratch,
                                 int batch, int n, void* stream);
int ccvpe_orientation_loss_f32(const float* ori, const float* gt_ori, const float* gt, float* loss,
                               float* scratch, int batch, int hw, void* stream);

/* -------------------------------------------------------------------------------------------
 * Train-mode pieces (efficientnet_pytorch/model.py:63,73,87,182,210: BatchNorm2d with batch statistics,
 * momentum 0.01, eps 1e-3; utils.py:129-154 drop_connect).  In train mode the conv kernels write their
 * raw output (ccvpe_conv_igemm_f32 with scale = shift = NULL, ccvpe_stem_conv_raw_f32,
 * ccvpe_dwconv_raw_f32), then:
 *   ccvpe_bn_stats_f32 : per-channel mean and BIASED variance of x [rows, channels] (shifted-sum partials per
 *       workgroup merged in two levels with Chan's formula: deterministic); if run_mean/run_var are given they
 *       are updated in place: run = (1-momentum)*run + momentum*(mean | UNBIASED variance).
 *       scratch: 3 * channels * ccvpe_bn_stats_nblk(rows) floats.
 *   ccvpe_bn_act_f32   : y = act((x-mean)/sqrt(var+eps)*gamma+beta) [* dc_scale[b]] [+ residual]; with
 *       se_partial != NULL also writes per-(sample, workgroup) channel sums of y
 *       [batch][ccvpe_bn_act_nblk(rows_per_sample)][channels] for ccvpe_se_gate_f32.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_stem_conv_raw_f32(const float* x_nchw, const float* w, float* y, int batch, int in_h, int in_w,
                            int circular, void* stream);
int ccvpe_dwconv_raw_f32(const float* x, const float* w, float* y, int batch, int in_h, int in_w, int channels,
                         int k, int stride, int circular, void* stream);
int ccvpe_bn_stats_nblk(int rows);
int ccvpe_bn_stats_f32(const float* x, int rows, int channels, float* mean, float* var, float* run_mean,
                       float* run_var, float momentum, float* scratch, void* stream);
int ccvpe_bn_act_nblk(int rows_per_sample);
int ccvpe_bn_act_f32(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                     float eps, int act, const float* residual, const float* dc_scale, float* y,
                     float* se_partial, int batch, int rows_per_sample, int channels, void* stream);

/* -------------------------------------------------------------------------------------------
 * Backward building blocks (wired into one torch.autograd.Function for the whole model by ccvpe_amd/train.py).
 *   ccvpe_conv_wgrad_f32: weight gradient of any dense conv of the path,
 *       dw[n][tap][c] = sum_pixels dy[pixel][n] * x[pixel*stride - pad + tap][c]     (layout O,kh,kw,I)
 *     x given as one or two concatenated NHWC sources (like the forward), dy [batch,Ho,Wo,ldy].
 *     scratch: ccvpe_conv_wgrad_scratch_floats(...) floats.  ConvTranspose2d(k2,s2): call it with
 *     x := the (high-res) output gradient, dy := the (low-res) forward input, k=2, stride=2.
 *   input gradients need no new kernel: they are ccvpe_conv_igemm_f32 calls with re-packed weights
 *     (1x1: W^T; 3x3: taps flipped, in/out swapped; deconv <-> conv 2x2 stride 2) — ccvpe_amd/backward.py.
 *   ccvpe_colsum_f32: per-channel column sums (bias gradients); scratch ceil(rows/256)*channels floats.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_conv_wgrad_tile(int n, int ncols);   /* (tile rows << 16) | tile columns the launch will use (reporting) */
int ccvpe_conv_wgrad_scratch_floats(int batch, int in_h, int in_w, int kh, int kw, int stride, int pad, int ctot,
                                    int n);
int ccvpe_conv_wgrad_f32(const float* src0, int c0, int ld0, const float* src1, int c1, int ld1, const float* dy,
                         int ldy, float* dw, float* scratch, int batch, int in_h, int in_w, int kh, int kw,
                         int stride, int pad, int n, void* stream);
/* the same launch also returns the conv's BIAS gradient dbias[n] = sum_pixels dy[pixel][n]: the first column tile of every row
 * tile adds up the dY pieces it stages anyway (one pass over dY instead of a ccvpe_colsum_f32 pass). */
int ccvpe_conv_wgrad_bias_f32(const float* src0, int c0, int ld0, const float* src1, int c1, int ld1, const float* dy,
                              int ldy, float* dw, float* dbias, float* scratch, int batch, int in_h, int in_w, int kh,
                              int kw, int stride, int pad, int n, void* stream);
/* 1x1 conv whose input is the squeeze-excite product x[b, px, c] * gate[b, c] (MBConv projection, model.py:118-121;
 * fewer than 128 output channels): the gate is applied while x is staged, the gated tensor is never materialised. */
int ccvpe_conv_wgrad_gated_f32(const float* x, int c, int ld, const float* gate, const float* dy, int ldy, float* dw,
                               float* scratch, int batch, int in_h, int in_w, int n, void* stream);
int ccvpe_colsum_f32(const float* x, int rows, int channels, int ld, float* out, float* scratch, void* stream);

/* -------------------------------------------------------------------------------------------
 * Backward of the train-mode EfficientNet pieces (csrc/train_bwd.hip).
 *   ccvpe_bn_act_bwd_f32 : backward of ccvpe_bn_act_f32 (batch-statistics BN + activation [* dc_scale]).
 *       dv is the gradient w.r.t. the consumer's input; with gate/dmean ([batch][channels]) the SE product
 *       and average-pool branches are folded in: du = dv*gate + dmean.  Writes dx (w.r.t. the raw conv
 *       output), dgamma, dbeta.  scratch: 2*channels*batch*ccvpe_bn_bwd_nblk(rows_per_sample) floats.
 *       The residual branch's gradient is dv itself.
 *   ccvpe_se_dgate_f32   : partial sums [batch][ccvpe_bn_bwd_nblk()][channels] of dv * u, u = act(bn(x)).
 *   ccvpe_se_bwd_f32     : the two SE 1x1 convs; consumes the forward squeeze partials and the dgate partials,
 *       writes dmean [batch][channels] (already / HW), dw1 [Cs][C], db1, dw2 [C][Cs], db2.
 *       scratch: 2*batch*(channels+squeezed) floats.
 *   ccvpe_dwconv_dgrad_f32 / ccvpe_dwconv_wgrad_f32 : depthwise conv input / weight gradients (dw [k][k][C]);
 *       wgrad scratch: batch*ccvpe_dwconv_wgrad_nblk()*k*k*channels floats.
 *   ccvpe_relu_bwd_f32   : dx = dy * (y > 0).
 * ----------------------------------------------------------------------------------------- */
int ccvpe_bn_bwd_nblk(int rows_per_sample);
int ccvpe_bn_act_bwd_f32(const float* x, const float* dv, const float* mean, const float* var, const float* gamma,
                         const float* beta, const float* gate, const float* dmean, const float* dc_scale, float eps,
                         int act, float* dx, float* dgamma, float* dbeta, float* scratch, int batch,
                         int rows_per_sample, int channels, void* stream);
/* Frozen BatchNorm (mean / var are constants of the step: the running statistics): the same arguments, preconditions and
 * scratch size as ccvpe_bn_act_bwd_f32, without the statistics-correction terms: g = (dv*gate + dmean) * dc_scale[b] * act'(z),
 * dx = gamma*istd*g, dbeta = sum g, dgamma = sum g*xhat.  One pass over (x, dv): dx and the per-workgroup partial sums come
 * out of the same kernel; the partials are merged in fixed order (no atomics). */
int ccvpe_bn_act_bwd_frozen_f32(const float* x, const float* dv, const float* mean, const float* var, const float* gamma,
                                const float* beta, const float* gate, const float* dmean, const float* dc_scale, float eps,
                                int act, float* dx, float* dgamma, float* dbeta, float* scratch, int batch,
                                int rows_per_sample, int channels, void* stream);
/* BatchNorm + squeeze-excite backward in two passes over (x, dv) instead of three (csrc/train_bwd.hip): the reduce pass
 * returns A [5][batch][channels] = per-(sample, channel) sums of (dv*u, dv*a', a', dv*a'*xhat, a'*xhat); A[0] is the SE gate
 * gradient (feed it to ccvpe_se_bwd_f32 as a one-row partial), and the apply call finishes dbeta / dgamma from A, gate and
 * dmean before writing dx.  scratch: batch * ccvpe_bn_bwd_nblk(rows_per_sample) * 5 * channels floats. */
int ccvpe_se_bn_bwd_reduce_f32(const float* x, const float* dv, const float* mean, const float* var, const float* gamma,
                               const float* beta, float eps, int act, float* A, float* scratch, int batch,
                               int rows_per_sample, int channels, void* stream);
int ccvpe_se_bn_bwd_apply_f32(const float* x, const float* dv, const float* mean, const float* var, const float* gamma,
                              const float* beta, const float* gate, const float* dmean, float eps, int act, const float* A,
                              float* dx, float* dgamma, float* dbeta, int batch, int rows_per_sample, int channels,
                              void* stream);
int ccvpe_se_dgate_f32(const float* x, const float* dv, const float* mean, const float* var, const float* gamma,
                       const float* beta, float eps, int act, float* part, int batch, int rows_per_sample,
                       int channels, void* stream);
int ccvpe_se_bwd_f32(const float* se_partial, int nblk, float inv_hw, const float* dgate_partial, int ndg,
                     const float* w1, const float* b1, const float* w2t, const float* b2, float* dmean, float* dw1,
                     float* db1, float* dw2, float* db2, float* scratch, int batch, int channels, int squeezed,
                     void* stream);
int ccvpe_dwconv_dgrad_f32(const float* dy, const float* w, float* dx, int batch, int in_h, int in_w, int channels,
                           int k, int stride, int circular, void* stream);
int ccvpe_dwconv_wgrad_nblk(int in_h, int in_w, int k, int stride);
int ccvpe_dwconv_wgrad_f32(const float* x, const float* dy, float* dw, float* scratch, int batch, int in_h, int in_w,
                           int channels, int k, int stride, int circular, void* stream);
int ccvpe_relu_bwd_f32(const float* y, const float* dy, float* dx, int n_elems, void* stream);
/* v = u * gate[b,c] materialised (the projection conv's weight gradient reads the gated tensor). */
int ccvpe_gate_mul_f32(const float* u, const float* gate, float* v, int batch, int rows_per_sample, int channels,
                       void* stream);

/* -------------------------------------------------------------------------------------------
 * Backward of the head / glue operators (csrc/heads_bwd.hip, csrc/matching_bwd.hip).
 *   ccvpe_softmax_bwd_f32   : dlogits = heatmap * (dheatmap - <heatmap, dheatmap>) [+ dlogits_direct]  (models.py:320)
 *   ccvpe_l2norm2_bwd_f32   : backward of F.normalize over the (cos, sin) pair (models.py:341); raw [B,2,HW]
 *   ccvpe_head_conv3x3_bwd_f32 : backward of ccvpe_head_conv3x3_f32 with normalize = 0: x [B,H,W,16] NHWC,
 *       dout [B,cout,H,W]; writes dx [B,H,W,16], dw [cout][3][3][16], dbias [cout].
 *       scratch: CCVPE_HEAD_BWD_SCRATCH floats.
 *   ccvpe_ground_descriptor_bwd_f32 : backward of ccvpe_ground_descriptor_f32: dout [B][w*sum(cd)] ->
 *       dy1 [B,h,w,ld] (pad columns zeroed), dwh [6][h], dbh [6].
 *   ccvpe_add_cols_f32      : dst[row, 0:channels] (+)= src[row, col_off : col_off+channels]  (skip-connection
 *       gradients are column slices of the decoder convs' input gradients).
 *   ccvpe_stem_conv_wgrad_f32 : stem weight gradient dw [3][3][3][32]; scratch: 864 * ccvpe_stem_wgrad_nblk() floats.
 *   ccvpe_match_level_bwd_f32 : backward of ccvpe_match_level_f32.  scores = the forward's scores; dscores
 *       [B,n_shifts,HW] (may be NULL) is the gradient arriving at the returned score volume, ddst [B,HW,ldo]
 *       the gradient arriving at dstx (normalised features, max column, tail columns).  Writes dx [B,HW,lddx]
 *       (first `channels` columns) and dg [B,ldg_out] (first L entries).  The max routes its gradient to the
 *       first maximal shift, as torch.max does.  scratch: batch * ccvpe_match_bwd_nblk(hw, batch, channels) * (L+1) floats.
 * ----------------------------------------------------------------------------------------- */
#define CCVPE_HEAD_WGRAD_BLOCKS 1024
#define CCVPE_HEAD_BWD_SCRATCH ((CCVPE_HEAD_WGRAD_BLOCKS + 1) * 2 * 145)
int ccvpe_softmax_bwd_f32(const float* heatmap, const float* dheatmap, const float* dlogits_direct, float* dlogits,
                          int rows, int n, void* stream);
int ccvpe_l2norm2_bwd_f32(const float* raw, const float* dout, float* draw, int batch, int hw, void* stream);
int ccvpe_head_conv3x3_bwd_f32(const float* x, const float* w, const float* dout, float* dx, float* dw, float* dbias,
                               float* scratch, int batch, int h, int wd, int cout, int relu_mask_x, void* stream);
int ccvpe_ground_descriptor_bwd_f32(const float* y1, int ld, const float* wh, const int* cd, const float* dout,
                                    float* dy1, float* dwh, float* dbh, int batch, int h, int w, void* stream);
int ccvpe_add_cols_f32(const float* src, int ld_src, int col_off, float* dst, int ld_dst, int channels, int rows,
                       int accumulate, void* stream);
int ccvpe_stem_wgrad_nblk(int batch, int in_h, int in_w);
int ccvpe_stem_conv_wgrad_f32(const float* x_nchw, const float* dy, float* dw, float* scratch, int batch, int in_h,
                              int in_w, int circular, void* stream);
int ccvpe_match_bwd_nblk(int hw, int batch, int channels);
int ccvpe_match_level_bwd_f32(const float* x, int ldx, const float* g, int ldg, int L, const int* shifts, int n_shifts,
                              int n_max, int n_tail, int stride, int window_offset, const float* scores, const float* dscores,
                              const float* ddst, int ldo, float* dx, int lddx, float* dg, int ldg_out, float* scratch,
                              int batch, int hw, int channels, void* stream);

/* Loss gradients w.r.t. the prediction (losses.py:4-29); dloss = upstream scalar gradient (device pointer).
 * infoNCE: `rows` is what ccvpe_infonce_loss_f32 wrote for the same (scores, labels); one pass, no statistics recomputed. */
int ccvpe_infonce_loss_bwd_f32(const float* scores, const float* labels, float temperature, const float* dloss,
                               const float* rows, float* dscores, int batch, int n, void* stream);
int ccvpe_cross_entropy_loss_bwd_f32(const float* logits, const float* labels, const float* dloss, float* dlogits,
                                     int batch, int n, void* stream);
int ccvpe_orientation_loss_bwd_f32(const float* ori, const float* gt_ori, const float* gt, const float* dloss,
                                   float* dori, int batch, int hw, void* stream);

/* -------------------------------------------------------------------------------------------
 * Training-step glue on the device (csrc/train_glue.hip).
 *   ccvpe_train_targets_f32: the ground-truth tensors of datasets.py:145-166 (VIGOR) / :470-501 (KITTI) and
 *     train_VIGOR.py:120-128 from 3 scalars per sample instead of 24 MB of host tensors:
 *       center_xy [B][2] = (cx, cy) with x_j = -W/2 + cx + j*W/(W-1), y_i = -H/2 + cy + i*H/(H-1)
 *                          (VIGOR: cx = col_offset, cy = -row_offset; KITTI: cx = x_offset, cy = y_offset)
 *       angle_deg [B] (wrapped into [0, 360) by the kernel);  n_bins 20 (VIGOR) / 16 (KITTI);  sigma 4
 *     writes gt [B,1,H,W], gt_norm [B,H*W] (= gt / sum gt), gt_ori [B,2,H,W] (cos, sin) and the six max-pooled
 *     orientation-binned label maps lab_l [B,n_bins,H/k,W/k], k = 64,32,16,8,4,2 (gt_with_ori is never materialised).
 *     scratch: batch * ccvpe_train_targets_nblk(h, w) floats.
 *   ccvpe_adam_step_f32: torch.optim.Adam (no weight decay / amsgrad; train_VIGOR.py:104) for ALL parameter tensors in
 *     one launch.  table [n_tensors][5] int64 device array of (param, grad, exp_avg, exp_avg_sq, numel) — a NULL grad
 *     skips the tensor; hyper [n_tensors][ccvpe_adam_hyper_floats()] fp32 device array, per tensor
 *     (lr / (1 - beta1^t), beta1, beta2, 1 - beta1, 1 - beta2, eps, sqrt(1 - beta2^t), 0) with t that tensor's own
 *     1-based step count (bias corrections and 1 - beta formed in double on the host, as torch does);
 *     chunk_tensor / chunk_off [n_chunks] map each workgroup to (tensor, chunk of ccvpe_adam_chunk_elems() elements);
 *     grad_scale multiplies every gradient on load (1 / world after a SUM all-reduce; 1 otherwise).
 * ----------------------------------------------------------------------------------------- */
int ccvpe_train_targets_nblk(int h, int w);
int ccvpe_train_targets_f32(const float* center_xy, const float* angle_deg, int n_bins, float sigma, float* gt,
                            float* gt_norm, float* gt_ori, float* lab1, float* lab2, float* lab3, float* lab4,
                            float* lab5, float* lab6, float* scratch, int batch, int h, int w, void* stream);
/* The same with the order of the orientation bins as a parameter: ascending = 0 is ccvpe_train_targets_f32 (VIGOR / KITTI: the
 * two bins are n - index and n - index - 1, datasets.py:156-161 / :489-494), ascending = 1 the Oxford RobotCar loader's
 * (datasets.py:340-347: bins index and index + 1, n - 1 wrapping to 0). */
int ccvpe_train_targets_ordered_f32(const float* center_xy, const float* angle_deg, int n_bins, int ascending, float sigma,
                                    float* gt, float* gt_norm, float* gt_ori, float* lab1, float* lab2, float* lab3,
                                    float* lab4, float* lab5, float* lab6, float* scratch, int batch, int h, int w,
                                    void* stream);
int ccvpe_adam_chunk_elems(void);
int ccvpe_adam_hyper_floats(void);
int ccvpe_adam_step_f32(const void* table, const float* hyper, const int* chunk_tensor, const int* chunk_off, int n_chunks,
                        float grad_scale, void* stream);

/* -------------------------------------------------------------------------------------------
 * Device-side optimizer (csrc/optim.hip): Adam / AdamW whose per-step numbers live in device memory, so a step needs no
 * host arithmetic, no upload and no read-back and captures into a hipGraph.  Same table and chunk maps as
 * ccvpe_adam_step_f32.  ccvpe_adam_device_layout(what): 0 = floats per derived hyper row, 1 = doubles per constant row,
 * 2 = floats in the scalar block.
 *   ccvpe_grad_sqnorm_f32: partials[c] = sum over chunk c of (grad_scale * g)^2 in a fixed order; a NULL grad gives 0.
 *   ccvpe_adam_prepare_f32 (one workgroup):
 *     scalars (total_norm, clip_coef, finite, skipped_steps): total_norm = sqrt(sum of the n_partials partials), the L2 norm
 *     of all gradients as torch.nn.utils.clip_grad_norm_ forms it; clip_coef = min(1, max_norm / (total_norm + 1e-6)), torch's
 *     formula (1 when max_norm <= 0); finite = 0 and skipped_steps += 1 when the norm is inf / NaN - the step is then SKIPPED
 *     (torch would scale by NaN).  n_partials == 0: no norm pass, total_norm 0, clip_coef 1, finite 1.
 *     Unless skipped, for every tensor with a non-NULL grad: steps[t] += 1 (fp32 counts, as torch's capturable optimizers keep
 *     them) and hyper[t] = (lr / (1 - beta1^t), beta1, beta2, 1 - beta1, 1 - beta2, eps, sqrt(1 - beta2^t), l2, decay, 0)
 *     formed in double from consts[t] = (lr, beta1, beta2, eps, weight_decay, decoupled), as torch.optim.Adam does with
 *     Python floats: l2 = weight_decay and decay = 1 (torch.optim.Adam: g += weight_decay * p) when decoupled == 0,
 *     l2 = 0 and decay = 1 - lr * weight_decay (torch.optim.AdamW: p *= 1 - lr * weight_decay) otherwise.
 *   ccvpe_adam_update_f32: ccvpe_adam_step_f32's arithmetic on rows of that layout with g scaled by
 *     grad_scale * clip_coef; g += l2 * p before the moments, p *= decay before the update; returns early for every tensor
 *     when finite == 0 (parameters, both moments and the step counts stay untouched).
 * ----------------------------------------------------------------------------------------- */
int ccvpe_adam_device_layout(int what);
int ccvpe_grad_sqnorm_f32(const void* table, const int* chunk_tensor, const int* chunk_off, int n_chunks, float grad_scale,
                          float* partials, void* stream);
int ccvpe_adam_prepare_f32(const void* table, const double* consts, float* steps, float* hyper, int n_tensors,
                           const float* partials, int n_partials, float max_norm, float* scalars, void* stream);
int ccvpe_adam_update_f32(const void* table, const float* hyper, const int* chunk_tensor, const int* chunk_off, int n_chunks,
                          float grad_scale, const float* scalars, void* stream);

/* -------------------------------------------------------------------------------------------
 * Input pipeline after JPEG decoding (csrc/preprocess.hip): transforms.Resize on a PIL image
 * (= Pillow's antialiased 8-bit BILINEAR resampler, reproduced bit for bit), ToTensor, Normalize
 * (train_VIGOR.py:57-70), torch.roll along W (datasets.py:112-121) and the FoV crop (train_VIGOR.py:177-178).
 *   src [in_h][in_w][3] uint8 (device), tmp [in_h][out_w][3] uint8 scratch, dst [3][out_h][keep_w] fp32 (one sample
 *   of the NCHW batch).  xbounds/ybounds [out][2] = (first source index, count), xcoef/ycoef [out][ksize] = Pillow's
 *   22-bit fixed-point coefficients (ccvpe_amd/preprocess.py builds them as precompute_coeffs() does).
 *   mean / std: HOST pointers to 3 floats.  roll: columns, as torch.roll's shift; keep_w <= out_w.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_preprocess_u8_f32(const unsigned char* src, int in_h, int in_w, const int* xbounds, const int* xcoef,
                            int xksize, const int* ybounds, const int* ycoef, int yksize, unsigned char* tmp, float* dst,
                            int out_h, int out_w, int keep_w, int roll, const float* mean, const float* stdv,
                            void* stream);

/* -------------------------------------------------------------------------------------------
 * Device-resident image cache (csrc/preprocess.hip; ccvpe_amd/cache.py): the per-file half of the input pipeline
 * (the Pillow-exact resize) kept as uint8 in HBM, and the per-epoch half (roll, FoV crop, ToTensor, Normalize) as ONE
 * launch per batch and side.
 *   resize_u8: the horizontal pass of the entry point above, then a vertical pass that writes the clipped bytes:
 *   dst_u8 [out_h][out_w][3] uint8 = PIL.Image.resize((out_w, out_h), BILINEAR) bit for bit.  Tables and tmp as above.
 *   gather_norm: srcs [batch] int64 (device) = DEVICE ADDRESSES of resized [h][w][3] uint8 images (a pointer table: the
 *   images may lie in any number of allocations), rolls [batch] int32 (device) = torch.roll shifts, any sign and size;
 *   dst [batch][3][h][keep_w] fp32, dst[b][c][y][x] = ((float)src_b[y][(x - roll_b) mod w][c] / 255 - mean[c]) / std[c]
 *   with the arithmetic of the entry point above (bit-identical to it).  mean / std: HOST pointers to 3 floats.
 *   keep_w <= w; batch == 0 succeeds without a launch; batch <= 65535.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_resize_u8(const unsigned char* src, int in_h, int in_w, const int* xbounds, const int* xcoef, int xksize,
                    const int* ybounds, const int* ycoef, int yksize, unsigned char* tmp, unsigned char* dst_u8,
                    int out_h, int out_w, void* stream);
int ccvpe_gather_norm_u8_f32(const long long* srcs, const int* rolls, int batch, int h, int w, int keep_w,
                             const float* mean, const float* stdv, float* dst, void* stream);

/* -------------------------------------------------------------------------------------------
 * Device-resident aerial map (csrc/preprocess.hip; Oxford RobotCar, the reference's datasets.py:296-330: crop an 800 x 800
 * patch of the one large map, Resize, ToTensor, Normalize): crop + Pillow-exact resize + normalise of a whole batch side in
 * ONE launch, with neither the window nor the horizontal intermediate written to memory.
 *   map [map_h][map_w][3] uint8 (device; any size — every byte offset is 64-bit); origins [batch][2] int32 (device) =
 *   (x0, y0) of each sample's box_h x box_w window, any sign, partly or wholly outside the map;
 *   W_b[i][j][c] = map[y0 + i][x0 + j][c] inside the map, else 0 (PIL.Image.crop of an RGB image; never read outside);
 *   dst [batch][3][out_h][out_w] fp32 = ccvpe_preprocess_u8_f32 of W_b (roll 0, keep_w = out_w), bit for bit.
 *   Tables: ccvpe_amd/preprocess.py resample_tables(box_w, out_w) / (box_h, out_h) on the device; the ksize arguments must be
 *   Pillow's for that geometry (2 * ceil(max(box / out, 1)) + 1), anything else is refused.  mean / std: HOST pointers.
 *   batch == 0 succeeds without a launch (tables may be null); batch <= 65535 (grid z); out_h <= 65535 * 16.
 *   Supported geometry: a 16 x 128 output tile stages floor(15 * box_h / out_h) + yksize + 1 window rows of 384 bytes in LDS
 *   and that must fit in 64 KB (170 rows): any enlargement, equal size, and vertical reductions up to box_h / out_h of
 *   about 9.8 (800 -> 512 stages 29 rows, a reduction by 4 stages 70); the horizontal factor is not limited.  A geometry
 *   beyond that is refused with CCVPE_EINVAL before anything is launched.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_window_resize_norm_u8_f32(const unsigned char* map, int map_h, int map_w, const int* origins, int batch, int box_h,
                                    int box_w, const int* xbounds, const int* xcoef, int xksize, const int* ybounds,
                                    const int* ycoef, int yksize, const float* mean, const float* stdv, float* dst, int out_h,
                                    int out_w, void* stream);

/* -------------------------------------------------------------------------------------------
 * KITTI aerial alignment (csrc/align.hip; the reference's datasets.py:443-464 / :577-596): PIL's rotate (NEAREST, 16.16
 * fixed point) -> two BILINEAR translations (float64, truncated) -> rotate -> centre crop, evaluated lazily per pixel
 * of the crop, bit-identical to Pillow.  ONE launch per batch.
 *   src: packed uint8 buffer (device) of src_bytes bytes holding the decoded [h][w][3] maps; offsets [batch] int64 =
 *   each sample's first byte; rows [batch][20] int64 = ccvpe_amd/align.py kitti_align_params (12 fixed-point integers,
 *   4 float64 bit patterns, w, h, left, top), sizes may differ per sample; dst [batch][crop_h][crop_w][3] uint8.
 *   A sample that does not fit in the buffer behind its offset is written as zeros and never read.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_kitti_align_u8(const unsigned char* src, long src_bytes, const long long* offsets, const long long* rows,
                         int batch, unsigned char* dst, int crop_h, int crop_w, void* stream);

/* -------------------------------------------------------------------------------------------
 * KITTI aerial alignment from device-resident maps, straight into the model's input (csrc/align.hip; ccvpe_amd/cache.py
 * raw slots): the same lazy chain, ONE launch per batch side, no uint8 crop in memory.
 *   srcs [batch] int64 (device) = DEVICE ADDRESSES of the decoded [h][w][3] uint8 maps (a pointer table: the maps may lie
 *   in any number of allocations, several rows may name the same address); rows [batch][20] int64 as above, w and h of
 *   each map from its row; dst [batch][3][crop_h][crop_w] fp32,
 *   dst[b][c][y][x] = ((float)byte / 255 - mean[c]) / std[c], byte = what ccvpe_kitti_align_u8 writes for that pixel, the
 *   fp32 arithmetic that of ccvpe_gather_norm_u8_f32 (bit-identical to align + gather).  mean / std: HOST pointers to 3 floats.
 *   A row whose address is 0, or whose w or h is outside 1..32767, is an all-zero crop and is never dereferenced; every
 *   other address must be readable for w * h * 3 bytes (the caller keeps the memory alive).
 *   batch == 0 succeeds without a launch (tables may be null); batch <= 65535 (grid z).
 * ----------------------------------------------------------------------------------------- */
int ccvpe_kitti_align_norm_u8_f32(const long long* srcs, const long long* rows, int batch, const float* mean,
                                  const float* stdv, float* dst, int crop_h, int crop_w, void* stream);

/* -------------------------------------------------------------------------------------------
 * bf16 storage variants (BASELINE configs C2 / C4).  Same kernels instantiated for bf16 NHWC
 * activations and bf16 packed weights (kpad a multiple of 32), fp32 accumulation on
 * v_mfma_f32_16x16x32_bf16, fp32 scale/shift/gate/bias, round-to-nearest-even on store.  Pointers
 * typed `void*` address bf16 data; everything else is as in the _f32 entry point of the same name.
 * In ccvpe_conv_desc src0/src1/w/residual/dst then address bf16 data; `out_f32` != 0 makes the GEMM
 * write fp32 instead (tensors handed to fp32 consumers: the ground-descriptor collapse).
 * Matching scores, heat-map logits and the orientation field are always fp32.
 * ----------------------------------------------------------------------------------------- */
int ccvpe_conv_igemm_bf16(const ccvpe_conv_desc* desc, int out_f32, void* stream);
int ccvpe_conv_igemm_splitk_bf16(const ccvpe_conv_desc* desc, int out_f32, float* scratch, void* stream);
int ccvpe_stem_conv_bf16(const float* x_nchw, const float* w, const float* scale, const float* shift, void* y,
                         int batch, int in_h, int in_w, int circular, void* stream);
int ccvpe_dwconv_bf16(const void* x, const float* w, const float* scale, const float* shift, void* y,
                      float* se_partial, int batch, int in_h, int in_w, int channels, int k, int stride,
                      int circular, void* stream);
int ccvpe_mbconv_front_bf16(const void* x, const void* w_exp, int kpad, const float* s0, const float* b0,
                            const float* w_dw, const float* s1, const float* b1, void* y, float* se_partial,
                            int batch, int in_h, int in_w, int cin, int mid, int k, int stride, int circular,
                            void* stream);
int ccvpe_match_level_bf16(const void* x, int ldx, const float* g, int ldg, int L, const int* shifts,
                           int n_shifts, int n_max, int n_tail, int stride, int window_offset, float* scores, void* dstx, int ldo,
                           int batch, int hw, int channels, void* stream);
int ccvpe_head_conv3x3_bf16(const void* x, const float* w, const float* bias, float* out_nchw, int batch, int h,
                            int w_, int cout, int normalize, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCVPE_HIP_H */
