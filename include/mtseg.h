/*
 * mtseg.h — C ABI of libmtseg_hip.so, the MI355X (gfx950) hot path of the 3D patch segmentation engine.
 *
 * The reference (MIC-DKFZ/MultiTalent, nnU-Net v1) has no FFI: its plugin surface is Python
 * (SURVEY.md §8b).  This ABI sits UNDER that surface: the Python modules that mirror
 * `Generic_UNet` / `FabiansUNet` / the trainers call these entry points through ctypes with raw
 * device pointers owned by the caller (torch), a hipStream_t and plain sizes.  No torch types,
 * no allocation, no synchronisation inside (mt_probe_device excepted, see there); every function returns 0
 * on success or a negative MT_E* code (text via mt_last_error(), thread-local).  Threading: launches are
 * re-entrant per stream and per device; since ABI 4 there is no mutable process-wide state (kernel selection is a field of the
 * problem struct, see "State" below) - only per-device caches of immutable properties and one-time kernel attributes.
 *
 * Layout: activations are NDHWC ("channels last"), fp32 or — in the mixed-precision mode, for the tensors the caller chooses —
 * bf16 (`dtype` = MT_BF16: the pointer then addresses 2-byte elements although it is typed `float*`), possibly a channel slice of a
 * wider buffer (channel stride `cs` in ELEMENTS, first channel folded into the pointer).  A "lazy activation" is a
 * raw conv output y plus per-(n,c) scale/shift and a LeakyReLU slope:
 *     a = lrelu_slope(y*scale + shift)         (InstanceNorm + LeakyReLU applied on load)
 * which is how `ConvDropoutNormNonlin.forward` (generic_UNet.py:66-70) is fused away.
 *
 * Each entry point cites the reference code it replaces (paths relative to the reference root).
 */
#ifndef MTSEG_H
#define MTSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MT_OK 0
#define MT_EINVAL (-1)  /* bad argument / unsupported shape */
#define MT_EWORKSPACE (-2) /* workspace too small */
#define MT_EHIP (-3)    /* HIP runtime error on launch */
#define MT_EUNSUPPORTED (-4) /* the device is not the one this library is built for (gfx950) */

#define MT_ABI_VERSION 4   /* 2: storage dtypes (mt_src_t.dtype, odtype fields, dtype arguments of the streaming kernels, mt_cast); 3: mt_pointwise_t.mma + mt_pointwise_pack_layout;
                            * 4: kernel selection is a FIELD of the problem (mt_conv3d_t.select / max_workgroups): mt_set_option and every MT_* environment
                            *    switch of the library are gone — no process-wide state besides per-device caches of immutable properties */
#define MT_MAX_CHUNKS 64

/* Storage type of an activation / gradient tensor in HBM.  fp32 is the parity path.  The mixed-precision mode (the reference's
 * autocast keeps conv inputs / outputs in half precision: MultiTalent_Trainer_DDP.py:340-354, network_trainer.py:400-402) stores
 * ACTIVATIONS as fp16 — the reference's own type: 11 significand bits, and the forward convolutions then multiply fp16 operands
 * (v_mfma_f32_32x32x16_f16) — and GRADIENTS as bf16 (fp32's exponent range: no loss scaling; the backward convolutions multiply
 * bf16 operands).  Values are rounded to nearest-even when stored and widened exactly when loaded; all arithmetic in between
 * (normalisation, statistics, accumulation, loss, optimizer) is fp32.  Not every kernel takes every combination: ask the
 * *_io_supported queries and convert with mt_cast where the answer is 0. */
#define MT_F32 0
#define MT_BF16 1
#define MT_F16 2

typedef void* mt_stream_t; /* hipStream_t */

/* One input source of a convolution: channel slice [0,C) of an NDHWC buffer with channel stride cs.
 * scale/shift: [N][C] per-sample affine applied on load (NULL = none); slope: LeakyReLU slope
 * applied after the affine (1.0f = identity). */
typedef struct {
  const float* ptr;
  int32_t cs;
  int32_t C;
  const float* scale;
  const float* shift;
  float slope;
  int32_t dtype;  /* MT_F32 | MT_BF16 | MT_F16: element type behind `ptr` (cs counts elements) */
} mt_src_t;

/* Fused statistics for the InstanceNorm + LeakyReLU backward that runs next (generic_UNet.py:63-64 in reverse).  A convolution that
 * is the LAST writer of a gradient tensor g = dL/d lrelu(IN(y)) (the backward-data of the layer's consumer) can emit, per block,
 * the two sums the normalisation backward needs over g,
 *     A = sum dz,   B = sum dz * zhat,      dz = g * lrelu'(z),  zhat = (y - mean) * rstd,  z = zhat * gamma + beta,
 * for its output channels [c0, c0 + C) (one of its two destinations) — the separate reduction pass over (g, y) disappears
 * (mt_inorm_lrelu_bwd with `part`).  The partials go to stats_part ([N][nsb][Cout][2], slot (.., c0 + c, 0 / 1) = A / B; channels
 * outside the range hold 0).  Supported by the kernels mt_conv3d_bwd_stats_supported() says yes to. */
typedef struct {
  const float* y;        /* raw forward output of the normalised layer [N, Do, Ho, Wo, ycs]; NULL = off */
  const float* mean;     /* [N][C] */
  const float* rstd;     /* [N][C] */
  const float* gamma;    /* [C] or NULL (1) */
  const float* beta;     /* [C] or NULL (0) */
  int32_t ycs, c0, C;
  float slope;
} mt_bwd_stats_t;

/* Convolution problem.  Forward conv (nn.Conv3d, generic_UNet.py:57,67; conv_blocks.py:49-85,116-213):
 *   out[n,o,co] = bias[co] + sum_{t,ci} in[n, o*S + t - P, ci] * W[t][ci][co]
 * with the input being the channel concatenation of src[0..nsrc) (torch.cat((x, skip), 1),
 * generic_UNet.py:392).  `dil` inserts zeros between stored input samples (virtual input coordinate
 * u maps to stored u/dil when divisible) — this is how the backward-data of a strided conv and
 * nothing else is expressed.  Weights are pre-packed by mt_pack_conv_weights. */
typedef struct {
  mt_src_t src[2];
  int32_t nsrc;
  int32_t N, Di, Hi, Wi;      /* stored input dims */
  int32_t dilD, dilH, dilW;   /* zero-insertion factor of the virtual input (1 or 2) */
  int32_t Do, Ho, Wo;         /* output dims */
  int32_t KD, KH, KW, SD, SH, SW, PD, PH, PW;
  int32_t Cin, Cout;
  const float* wpack;         /* packed weights (mt_pack_conv_weights, ck = MT_CONV_CK) */
  const float* bias;          /* [Cout] or NULL */
  float* out0; int32_t ocs0;  /* channels [0,csplit) -> out0[... * ocs0 + co] */
  float* out1; int32_t ocs1;  /* channels [csplit,Cout) -> out1[... * ocs1 + (co - csplit)] (may be NULL if csplit>=Cout) */
  int32_t csplit;
  int32_t accumulate;         /* 1: out += result (gradient accumulation on skip connections) */
  float* stats_part;          /* NULL or [N][nsb][Cout][2] per-block (sum, sumsq) partials, nsb = mt_conv3d_stats_blocks() */
  /* Strided output placement (0 = dense): logical output position o is written at o*os + oo of a tensor with spatial dims
   * (OD,OH,OW).  Used by the backward-data of a strided conv, which is computed as one exact stride-1 convolution per
   * parity class of the input position instead of a convolution over a zero-inserted gradient. */
  int32_t OD, OH, OW, osD, osH, osW, ooD, ooH, ooW;
  int32_t mma;                /* matrix input type of the convolution: 0 fp32 (exact), 1 bf16 inputs with fp32 accumulation
                                 (mixed precision, the reference's autocast mode); packed weights must match (mt_conv3d_pack_layout) */
  int32_t odtype;             /* MT_F32 | MT_BF16 | MT_F16: element type of out0 / out1 (ocs0 / ocs1 count elements); statistics are taken from
                                 the values as stored */
  mt_bwd_stats_t bstats;      /* bstats.y != NULL: fused first pass of the NEXT InstanceNorm backward (see mt_bwd_stats_t) */
  uint32_t select;            /* ABI 4: kernel selection of THIS problem, 2-bit fields MT_SEL_* (0 = the library's policy everywhere).  The queries
                                 (mt_conv3d_ck, _pack_layout, _stats_blocks, _kernel_name, *_io_supported, *_workspace) and the launch must see the same value. */
  int32_t max_workgroups;     /* ABI 4: > 0 caps the workers of the persistent kernels (conv_wino8p: per output-channel tile; conv_x16, conv_bwdw_tr16: total)
                                 — tests make a worker walk several tiles of a small problem; 0 = fill the chip */
} mt_conv3d_t;

/* mt_conv3d_t.select: which kernel FAMILIES may serve the problem.  All families compute the same convolution (fp32: to rounding of the
 * summation order; mma == 1: the 16-bit matrix kernels round the operands); the policy (MT_SEL_DEFAULT) takes a specialised kernel where
 * its grid fills the chip.  Tests force a family on small shapes (MT_SEL_FORCE) or exclude it (MT_SEL_OFF) to compare two kernels on the
 * same problem; the A/B tools do the same over whole steps. */
#define MT_SEL_DEFAULT 0u
#define MT_SEL_OFF 1u
#define MT_SEL_FORCE 2u
#define MT_SEL_WINO 0        /* shift: Winograd F(2x2x2, 3x3x3) forward / backward-data (conv_wino8p_kernel) */
#define MT_SEL_M16 2         /* 16-bit matrix kernels of mma == 1 problems (conv_bf16_kernel, conv_x16_kernel; OFF = the fp32 kernels) */
#define MT_SEL_X16 4         /* conv_x16_kernel among them (DEFAULT: where it measured faster; FORCE: wherever eligible) */
#define MT_SEL_TAPSPLIT 6    /* conv_tapsplit_kernel on under-filled grids (FORCE: the strided form also on well-filled grids) */
#define MT_SEL_BWDW_WINO 8   /* F(3x3, 2x2) backward-weight kernels (3x3x3 and 1x3x3) */
#define MT_SEL_BWDW_TR16 10  /* conv_bwdw_tr16_kernel (16-bit X, bf16 dY) */
#define MT_SEL_BWDW_CW 12    /* cout tiles per workgroup of the tiled backward-weight kernels: 0 = up to 4 where a workgroup walks enough tiles,
                                1 = one, 2 = at most two, 3 = up to 4 also on small problems */
#define MT_SEL_GET(sel, shift) (((sel) >> (shift)) & 3u)

const char* mt_last_error(void);
int mt_abi_version(void);

/* ---- weight packing ------------------------------------------------------------------------
 * Packs W_eff[tap][ci][co] = w[ci*s_ci + co*s_co + kd'*s_kd + kh'*s_kh + kw'*s_kw] (k' = K-1-k when
 * flip) into the MFMA B-fragment order [ntile][chunk][tap][ck/2][64] used by the conv kernels, where
 * the input channels are split into chunks of at most `ck` channels that never straddle the two
 * sources (C0 | C1).  Returns number of floats via *packed_floats (query with dst == NULL). */
int mt_pack_conv_weights(const float* w, float* dst, size_t* packed_floats,
                         int C0, int C1, int Cout, int KD, int KH, int KW,
                         long s_ci, long s_co, long s_kd, long s_kh, long s_kw, int flip, int ck,
                         int layout /* 1: all MFMA kernels ([kp/4][lane][4], pair (kp, ck/2+kp)); mt_pointwise_fwd takes ck = 16;
                                       0: legacy [kp][lane], pair (2kp,2kp+1); 2: Winograd F(2x2x2,3x3x3) U = G g G^T (ck = 8);
                                       3: bf16 B fragments of v_mfma_f32_32x32x16_bf16, [tap][lane][8 bf16] (ck = 16), RNE */,
                         const int32_t* tapmap /* NULL, or {tbD,tsD,tbH,tsH,tbW,tsW}: packed tap j of dim d takes source
                                                  tap tb + ts*j (overrides flip) — sub-kernels of the parity classes */,
                         mt_stream_t stream);

/* ---- convolution (N1/N2/N5 forward, and backward-data through flipped weights) --------------- */
int mt_conv3d_fwd(const mt_conv3d_t* p, mt_stream_t stream);
int mt_conv3d_stats_blocks(const mt_conv3d_t* p); /* spatial blocks per sample (size of stats_part dim 1) */
int mt_conv3d_ck(const mt_conv3d_t* p);           /* channel chunk the kernel will use (pack weights with it) */
/* Batched packing: all layers of one optimizer step in one launch.  mt_pack_desc_fill writes one opaque descriptor
 * (mt_pack_desc_size() bytes, same arguments as mt_pack_conv_weights) into HOST memory; the caller uploads the table once and
 * calls mt_pack_batched(table_on_device, n) every step — the descriptors stay valid while the weight and destination buffers
 * do. */
size_t mt_pack_desc_size(void);
int mt_pack_desc_fill(void* desc, const float* w, float* dst, int C0, int C1, int Cout, int KD, int KH, int KW, long s_ci,
                      long s_co, long s_kd, long s_kh, long s_kw, int flip, int ck, int layout, const int32_t* tapmap);
int mt_pack_batched(const void* descs_device, int n, mt_stream_t stream);

/* Backward-data of a strided 3x3x3 convolution (pad 1, stride (2,2,2) or (1,2,2)) in one launch — replaces autograd's
 * conv_transpose for the strided stage convs (generic_UNet.py:263-278 `first_stride`, generic_modular_UNet.py:69-77).
 * p carries the FORWARD geometry: Di/Hi/Wi = X dims, Do/Ho/Wo = Y dims, K, S, P, Cin, Cout; src[0] = dY (C = Cout, may be lazy);
 * out0/ocs0 = dX (Cin channels), accumulate adds to it.  wpack = mt_pack_conv_weights(w, C0 = Cout, C1 = 0, Cout_arg = Cin,
 * kernel 3x3x3, strides with the ci/co roles swapped, flip = 0, ck = 16, layout 1).  Each of the 27 taps is one MFMA block
 * into the accumulator of the parity class (x mod stride) it reaches: no work on inserted zeros. */
int mt_conv3d_bwd_data_strided(const mt_conv3d_t* p, mt_stream_t stream);
int mt_conv3d_bwd_data_strided_supported(const mt_conv3d_t* p);   /* 1 when the geometry is handled, else 0 */
int mt_conv3d_bwd_data_strided_pack_layout(const mt_conv3d_t* p); /* `layout` of its packed weights: 1, or 3 (bf16) when p->mma == 1 */
/* Storage types: 1 when the kernel that serves p takes p->src[*].dtype / p->odtype natively (all-fp32: always).  0: convert the
 * operands with mt_cast (the launch itself refuses with MT_EINVAL).  Same question for the other convolution entry points. */
int mt_conv3d_io_supported(const mt_conv3d_t* p);
int mt_conv3d_bwd_data_strided_io_supported(const mt_conv3d_t* p);
int mt_conv3d_bwd_weight_io_supported(const mt_conv3d_t* p, const mt_src_t* ysrc);

/* State.  The library keeps NO mutable process-wide state (ABI 4): which kernel serves a problem is a function of the problem struct
 * alone (geometry, storage types, mma, select, max_workgroups), launches are re-entrant across host threads and streams, and memory
 * (outputs, workspaces, statistics partials) is caller-owned.  What it caches is immutable per DEVICE: a kernel's raised dynamic-LDS
 * limit and the CU count that sizes persistent grids, keyed by the current HIP device (one process may drive several GPUs).
 * Rounds 1 - 5 had 39 MT_* environment switches and mt_set_option in here; the A/Bs they served are closed, the losing
 * kernels are deleted or unreachable, and the families tests still compare are the MT_SEL_* fields above.
 * The HOST side above this ABI (multitalent_amd/) reads four environment variables, and no others: MT_SELECT ("x16=off,wino=force,...":
 * default mt_conv3d_t.select of the process, for A/B runs of whole steps), MT_LIB_VARIANT (file name of an instrumented build of this
 * library), MT_FORCE_REDUCER (1: the bucketed side-stream all-reduce also at world size 1) and MT_BWDW_STREAMS (0: weight gradients on
 * the compute stream, which the per-kernel profiles need; results are bit-identical).  bench.py adds MT_BENCH_ONE_GPU (all ranks on
 * cuda:0 over gloo).  The experiment switches of rounds 2 - 6 and the opt-in HIP-graph step are gone (DESIGN.md 0, 3 and 6 keep
 * their measurements).  Which workgroup computes which tile (block id -> XCD -> tile order) is fixed; results do not
 * depend on it. */

/* Device probe (SYNCHRONOUS, call once per device before the first launch; the Python binding does so when it loads the
 * library): checks that the current device is gfx950 and that raw buffer loads behave the way the vector-load kernels assume —
 * a dword-aligned buffer_load_dwordx4 returns its four dwords, and a load that straddles num_records returns the in-range dwords
 * and zeros for the rest.  `scratch`: >= 32 KiB of device memory owned by the caller.  *vector_loads_ok = 1 / 0; `arch` receives
 * the gcnArchName.  Returns MT_EUNSUPPORTED on a non-gfx950 device. */
int mt_probe_device(void* scratch, size_t scratch_bytes, int* vector_loads_ok, char* arch, size_t arch_len, mt_stream_t stream);
int mt_conv3d_pack_layout(const mt_conv3d_t* p);   /* `layout` for mt_pack_conv_weights: 1; 2 when the Winograd kernel serves p; 3 (bf16) when p->mma == 1 and the bf16 kernel does */
int mt_conv3d_kernel_name(const mt_conv3d_t* p, char* buf, size_t n); /* device kernel that will run (profiler name) */
int mt_conv3d_bwd_stats_supported(const mt_conv3d_t* p); /* 1 when the kernel that serves p (geometry, ignoring p->bstats) honours p->bstats */
/* the same for mt_conv3d_bwd_weight(p, ysrc, ...) and mt_conv3d_bwd_data_strided(p): which kernel family the dispatcher picks
 * (tests assert that full-size problems run on the Winograd / strided / stem kernels; bench.py groups its timings by it) */
int mt_conv3d_bwd_weight_kernel_name(const mt_conv3d_t* p, const mt_src_t* ysrc, char* buf, size_t n);
int mt_conv3d_bwd_data_strided_kernel_name(const mt_conv3d_t* p, char* buf, size_t n);
/* mt_pointwise_kernel_name, mt_pointwise_launch_shape and mt_head_bwd_kernel_name, the same for mt_pointwise_fwd and mt_head_bwd, are
 * declared below, after mt_pointwise_t. */

/* ---- backward-weight -------------------------------------------------------------------------
 * dW[tap][ci][co] = sum_{n,o} X[n, o*S + t - P, ci] * Y[n, o, co]   (autograd of nn.Conv3d /
 * nn.ConvTranspose3d weights).  X is described by p->src (lazy activations allowed), Y by ysrc
 * (N,Do,Ho,Wo from p).  Result is written (or accumulated) into dw with the given element strides,
 * i.e. directly in the torch parameter layout.  Workspace: query mt_conv3d_bwd_weight_workspace. */
size_t mt_conv3d_bwd_weight_workspace(const mt_conv3d_t* p);
int mt_conv3d_bwd_weight(const mt_conv3d_t* p, const mt_src_t* ysrc, float* dw,
                         long s_ci, long s_co, long s_kd, long s_kh, long s_kw, int accumulate,
                         void* workspace, size_t workspace_bytes, mt_stream_t stream);

/* ---- pointwise / transposed convolution -----------------------------------------------------
 * Base grid [N][Db][Hb][Wb].  in voxel = base*si (gather), out voxel = base*so + tap (scatter, taps
 * = prod(so)).  si=so=1: 1x1x1 conv (seg heads generic_UNet.py:349-351; backward-data with packed
 * transposed weights).  si=2: strided 1x1x1 skip projection (conv_blocks.py:192-197).
 * so=pool kernel: nn.ConvTranspose3d with kernel==stride, bias=False (generic_UNet.py:335-336),
 * written straight into the concat buffer through ocs. */
typedef struct {
  mt_src_t src;
  int32_t N, Db, Hb, Wb;
  int32_t Di, Hi, Wi;          /* stored input dims (base*si must be inside) */
  int32_t siD, siH, siW;
  int32_t soD, soH, soW;
  int32_t Cin, Cout;
  const float* wpack;  /* mt_pack_conv_weights(C0=Cin, C1=0, taps = so, ck = Cin rounded up to even) */
  const float* bias;   /* [Cout] or NULL */
  float* out; int32_t ocs;
  int32_t accumulate;
  float* stats_part;   /* NULL or [N][nsb][Cout][2] */
  int32_t odtype;      /* MT_F32 | MT_BF16 | MT_F16: element type of `out` */
  int32_t scatter;     /* 0: all prod(so) taps (transposed convolution).  1: ONLY tap (0,0,0) — out[base*so] (+)= W x in[base], one packed
                          tap: the backward-data of a strided 1x1x1 convolution (conv_blocks.py:159-165); the other output positions are
                          not touched (the caller zero-fills or accumulates) */
  int32_t mma;         /* ABI v3.  0: fp32 products.  1 (mixed precision): fp16 products where the source is stored in fp16 and the kernel
                          that serves the problem has the 16-bit matrix form — the packed weights must then be in the layout
                          mt_pointwise_pack_layout(p) returns (4 instead of 1) */
} mt_pointwise_t;
int mt_pointwise_fwd(const mt_pointwise_t* p, mt_stream_t stream);
int mt_pointwise_stats_blocks(const mt_pointwise_t* p);
int mt_pointwise_io_supported(const mt_pointwise_t* p);
/* pack layout (mt_pack_conv_weights, ck = 16) of the weights this problem's launch reads: 1, or 4 (fp16 B fragments) when p->mma == 1
 * and the launch multiplies in fp16 (transposed convolutions and 33..64-channel heads over fp16 activations). */
int mt_pointwise_pack_layout(const mt_pointwise_t* p);   /* 1 when p->src.dtype / p->odtype are read / written natively (see MT_F16) */
/* The kernel instance mt_pointwise_fwd(p) launches (profiler name, e.g. "pw_fast_kernel<4, 2, 2, true>": taps per workgroup, source and
 * destination storage type, fp16 products) and the return code the launch would give, without launching: a problem the launch refuses is
 * refused here with the same code.  mt_pointwise_launch_shape adds what a template name does not show: grid x, y, z and the store form
 * of the transposed convolutions (0 dword stores, 1 16-byte pieces per voxel, 2 one linear run per tap pair); eight taps without
 * statistics run as <4, ...> with z = 2.  Neither touches a device. */
int mt_pointwise_kernel_name(const mt_pointwise_t* p, char* buf, size_t n);
int mt_pointwise_launch_shape(const mt_pointwise_t* p, int32_t shape[4]);
/* Backward of a 1x1x1 segmentation head (generic_UNet.py:349-351, generic_modular_UNet.py:244,251: seg_outputs / deep_supervision_outputs)
 * in ONE pass over (x, dY):  dX[n,v,ci] (+)= sum_co dY[n,v,co] W[co,ci] (gradient w.r.t. the lazily ACTIVATED head input),
 * dW[co*s_co + ci*s_ci] (+)= sum_{n,v} act(x)[n,v,ci] dY[n,v,co], dbias[co] (+)= sum dY.  Cin, Cout <= 64; mt_head_bwd_supported says
 * where it beats the separate kernels (Cin <= 32: the full-resolution heads).
 * x: the head's input (lazy activation allowed); dy [N][V][dycs]; wpack_bwd = mt_pack_conv_weights(w, C0 = Cout, C1 = 0, Cout' = Cin,
 * 1x1x1, strides with ci/co swapped, flip 0, ck 16, layout 1) — the packing mt_pointwise_fwd takes for the same backward-data.
 * *dbias_done = 1 when dbias was produced (Cin not a multiple of 32: a spare MFMA row carries 1.0), else the caller sums dY
 * (mt_channel_sum).  ws: mt_head_bwd_workspace bytes (per-wave partials, summed in fp64 in a fixed order). */
int mt_head_bwd_supported(int Cin, int Cout);
size_t mt_head_bwd_workspace(int N, long V, int Cin, int Cout);
int mt_head_bwd(const mt_src_t* x, const float* dy, int dycs, int N, long V, int Cin, int Cout, const float* wpack_bwd,
                float* dx, int dxcs, int dxdtype /* storage type of dx: fp32, or bf16 with a 16-bit x */, int accumulate_dx, float* dw,
                long s_ci, long s_co, float* dbias, int accumulate_dw, int* dbias_done, void* ws, size_t ws_bytes, mt_stream_t stream);
int mt_head_bwd_io_supported(int xdtype, int xcs, int dxdtype, int dxcs, int Cin, int Cout);
/* the main kernel instance mt_head_bwd launches for these operands and, in *dbias_done (may be NULL), what the launch would report;
 * returns the launch's code for what it can see (no dy / dx / dw / workspace here).  Touches no device. */
int mt_head_bwd_kernel_name(const mt_src_t* x, int dycs, int N, long V, int Cin, int Cout, int dxcs, int dxdtype, char* buf, size_t n,
                            int* dbias_done);


/* ---- InstanceNorm3d(eps, affine) + LeakyReLU (generic_UNet.py:63-64,69-70) ------------------- */
/* partials [N][nsb][C][2] -> mean,rstd,scale,shift each [N][C]; scale = gamma*rstd, shift = beta - mean*scale */
int mt_inorm_finalize(const float* part, int N, int nsb, int C, double count, const float* gamma,
                      const float* beta, float eps, float* mean, float* rstd, float* scale, float* shift,
                      mt_stream_t stream);
/* materialise a = lrelu(y*scale+shift) (+ optional residual add BEFORE the lrelu: conv_blocks.py:201-213) */
int mt_inorm_lrelu_apply(const float* y, int ycs, const float* scale, const float* shift, float slope,
                         const float* res, int rcs, const float* rscale, const float* rshift, float rslope,
                         float* out, int ocs, int N, long V, int C, int dtype /* storage type of y, res and out */, mt_stream_t stream);
/* Backward of out = lrelu(IN(y)): given g = dL/dout (in place), produce dy in place, plus
 * dgamma[C] += , dbeta[C] +=, dbias[C] (= sum dy, may be NULL).  ws: mt_inorm_bwd_workspace bytes.
 * part != NULL: the first pass (sum dz, sum dz zhat per block) was fused into the convolution that produced g
 * (mt_conv3d_t.bstats): part = its stats_part [N][part_nblk][part_cs][2], this layer's channels at columns part_c0 ..; the
 * reduction pass over (g, y) is skipped.  part == NULL: computed here. */
size_t mt_inorm_bwd_workspace(int N, long V, int C);
int mt_inorm_lrelu_bwd(float* g, int gcs, const float* y, int ycs, const float* mean, const float* rstd,
                       const float* gamma, const float* beta, float slope, int N, long V, int C,
                       float* dgamma, float* dbeta, float* dbias, const float* part, int part_nblk, int part_cs, int part_c0,
                       void* ws, size_t ws_bytes, int gdtype, int ydtype /* storage types of g and of y */, mt_stream_t stream);
/* g *= lrelu'(y*scale+shift) in place, optionally also writes a copy (residual branch gradient) */
int mt_lrelu_bwd(float* g, int gcs, const float* y, int ycs, const float* scale, const float* shift,
                 float slope, const float* y2, int y2cs, const float* scale2, const float* shift2,
                 float slope2, float* gcopy, int gcopycs, int N, long V, int C, int gdtype /* of g, gcopy */, int ydtype /* of y, y2 */,
                 mt_stream_t stream);
/* mt_lrelu_bwd on dense tensors (channel stride == C) that also emits the first pass of the NEXT InstanceNorm backward: in a residual
 * block out = lrelu(IN(y) + residual) (conv_blocks.py:201-213) the masked gradient g' is the gradient of IN(y), so
 * part[n][blk][c] = (sum g', sum g' * (y - mean) * rstd) over the block's voxels — mt_inorm_lrelu_bwd(part, part_nblk =
 * mt_lrelu_bwd_stats_blocks(V, C), part_cs = C, part_c0 = 0) then skips its own reduction over (g', y).  mean / rstd: [N][C] of that
 * norm.  mt_lrelu_bwd_stats_blocks returns 0 for shapes this path does not take (C % 4 != 0, C > 1024). */
int mt_lrelu_bwd_stats_blocks(long V, int C);
int mt_lrelu_bwd_stats(float* g, const float* y, const float* scale, const float* shift, float slope,
                       const float* y2, const float* scale2, const float* shift2, float slope2, float* gcopy,
                       const float* mean, const float* rstd, float* part, int N, long V, int C, int gdtype /* of g, gcopy */,
                       int ydtype /* of y, y2 */, mt_stream_t stream);
/* Which kernel instance a streaming launch takes (additions to ABI 4; the launch and the query read one decision).  The arguments are
 * the launch's own, as far as the decision reads them; of a pointer only NULL-ness and alignment are read, so no memory needs to stand
 * behind it, and no device is touched.  buf receives the name as a profiler prints it ("inorm_bwd_fast_kernel<2, true, 0, 0>",
 * "inorm_bwd_small_kernel<8, 2, 1>", "inorm_apply_kernel": the strided kernels are no templates).  Returns what the launch would
 * return for these arguments (MT_EINVAL where it refuses them).
 * mt_inorm_lrelu_bwd_kernel_name names the kernel that writes dy; *own_reduce (may be NULL) = 1 when the launcher's own reduction pass
 * over (g, y) runs before it (0 with external partials, and for the one-launch small kernel, which reduces in itself); *block (may be
 * NULL) = threads per workgroup of the named kernel (256 .. 1024 for the small kernel). */
int mt_inorm_lrelu_apply_kernel_name(const float* y, int ycs, const float* res, int rcs, const float* out, int ocs, int N, long V, int C,
                                     int dtype, char* buf, size_t n);
int mt_inorm_lrelu_bwd_kernel_name(const float* g, int gcs, const float* y, int ycs, const float* mean, const float* rstd, int N, long V, int C,
                                   const float* part, int part_nblk, int part_cs, int part_c0, int gdtype, int ydtype,
                                   char* buf, size_t n, int* own_reduce, int* block);
int mt_lrelu_bwd_kernel_name(const float* g, int gcs, const float* y, int ycs, const float* y2, int y2cs, const float* gcopy, int gcopycs,
                             int N, long V, int C, int gdtype, int ydtype, char* buf, size_t n);
int mt_lrelu_bwd_stats_kernel_name(const float* g, const float* y, const float* y2, const float* gcopy, const float* mean, const float* rstd,
                                   const float* part, int N, long V, int C, int gdtype, int ydtype, char* buf, size_t n);
/* per-channel sum over all voxels: out[C] (+)= sum_{n,v} x[n,v,c]  (bias gradients of heads) */
size_t mt_channel_sum_workspace(int N, long V, int C);
int mt_channel_sum(const float* x, int xcs, int N, long V, int C, float* out, int accumulate,
                   void* ws, size_t ws_bytes, int dtype /* storage type of x */, mt_stream_t stream);
/* Storage-type conversion, the boundary op of the mixed-precision mode: dst[r][c] (+)= src[r][c] for `rows` voxels (all samples) of
 * C channels, each side with its own storage type (MT_F32 | MT_BF16 | MT_F16) and channel stride in elements.  accumulate adds in fp32 and
 * rounds once.  A kernel that does not take a tensor's storage type (the *_io_supported queries) works on such a copy. */
int mt_cast(const void* src, int scs, int sdtype, void* dst, int dcs, int ddtype, long rows, int C, int accumulate,
            mt_stream_t stream);

/* ---- losses --------------------------------------------------------------------------------- */
/* MultiTalent loss for one deep-supervision level (MultiTalent_Trainer_DDP.py:544-623):
 * logits [B][V][C=47 (cs)], target [B][V] float label map, valid[B] = 64-bit mask of valid output
 * channels, lut[C] = 64-bit mask over label values belonging to each channel's region
 * (Task100_MultiTalent.py:118-166).  Forward: stats[B][C][4] = (bce_sum, tp, fp, fn).
 * Backward = exact vector-Jacobian product of the forward: given gstats[B][C][4] = dLoss/dstats,
 * dlogits[b,v,c] = valid * ( g0*(sigmoid-y) + sigmoid*(1-sigmoid)*( y*(g1-g3) + (1-y)*g2 ) ), 0 for invalid
 * channels — written once (the reference's autograd zero-fills a full tensor per region). */
int mt_multitalent_loss_fwd(const float* logits, int cs, const float* target, int B, long V, int C,
                            const uint64_t* valid, const uint64_t* lut, float* stats, void* ws,
                            size_t ws_bytes, mt_stream_t stream);
size_t mt_loss_workspace(int B, long V, int C);
int mt_multitalent_loss_bwd(const float* logits, int cs, const float* target, int B, long V, int C,
                            const uint64_t* valid, const uint64_t* lut, const float* gstats,
                            float* dlogits, int dcs, mt_stream_t stream);
/* Online evaluation of the MultiTalent trainers (MultiTalent_Trainer_DDP.py:372-398): hard predictions sigmoid(x) > 0.5 of the
 * full-resolution logits against the region masks; stats[B][C][3] = exact counts (tp, fp, fn) of the channels valid for the
 * sample's dataset, 0 elsewhere.  ws: mt_hard_stats_workspace(B, C) bytes (64-bit counters, integer atomics: order-free). */
int mt_multitalent_hard_stats(const float* logits, int cs, const float* target, int B, long V, int C,
                              const uint64_t* valid, const uint64_t* lut, float* stats, void* ws, size_t ws_bytes,
                              mt_stream_t stream);
size_t mt_hard_stats_workspace(int B, int C);
/* Softmax Dice+CE for one level (dice_loss.py:100-195,488-545; crossentropy.py:4-11):
 * stats[B][C][4] = (ce_sum (only c=0 slot used, the others 0), tp, fp, fn).  A label outside 0..C-1 is no class: a zero one-hot
 * row, no CE term, and no CE gradient in the backward. */
int mt_softmax_dice_ce_fwd(const float* logits, int cs, const float* target, int B, long V, int C,
                           float* stats, void* ws, size_t ws_bytes, mt_stream_t stream);
int mt_softmax_dice_ce_bwd(const float* logits, int cs, const float* target, int B, long V, int C,
                           const float* gstats /* [B][C][4], slot (b,0,0) = dLoss/dce_sum[b] */,
                           float* dlogits, int dcs, mt_stream_t stream);
/* The loss combination on top of the per-level statistics, value and gradient in one launch (the reference forms it with a few
 * dozen autograd operations on [B, C] tensors: MultiTalent_Trainer_DDP.py:598-623; dice_loss.py:150-183 + deep_supervision.py:37-42;
 * nnUNetTrainerV2_DDP.py:262-282).  stats [L][B][C][4] as written by the *_fwd calls of the L levels; dice [L][B][C][dice_stride] =
 * (tp, fp, fn, ...) the Dice ratios are formed from: stats + 1 with stride 4, or the sum of the statistics over ranks with stride 3.
 *   loss = sum_l ce_coef[l] * sum_{b, c in CE set} stats[l,b,c,0]  -  sum_l dice_coef[l] * sum_entries r,
 *   r = (2 tp + smooth_num) / max(2 tp + fp + fn + smooth_den + den_eps, clamp_min)   over channels c >= c0,
 * flags: MT_LOSS_CE_ALL_CHANNELS (else channel 0 carries the level's CE sum), MT_LOSS_DICE_OVER_BATCH (tp / fp / fn summed over b
 * before the ratio).  ce_coef, dice_coef: device vectors [L].  out3 = (loss, CE part, Dice part); gstats [L][B][C][4] =
 * dLoss/d(local stats), the argument of the *_bwd calls; its Dice part is multiplied by dice_grad_scale (the world size when `dice`
 * is the sum over ranks: the backward of the reference's all-gather sums the ranks' identical gradients, distributed.py:63-73). */
#define MT_LOSS_CE_ALL_CHANNELS 1
#define MT_LOSS_DICE_OVER_BATCH 2
int mt_loss_combine(const float* stats, const float* dice, int dice_stride, int L, int B, int C, const float* ce_coef,
                    const float* dice_coef, int flags, int c0, float smooth_num, float smooth_den, float den_eps, float clamp_min,
                    float dice_grad_scale, float* out3, float* gstats, mt_stream_t stream);
/* Which kernel a loss launch takes (additions to ABI 4; the launch and the query read one decision, no device is touched, and of a
 * pointer only NULL-ness and alignment are read).  buf receives the name as a profiler prints it; a query returns what the launch
 * returns for the arguments it sees (MT_EINVAL where the launch refuses them).
 *   mt_multitalent_loss_fwd: "mt_loss_fwd_sparse_kernel" (cs == C) | "mt_loss_fwd_kernel".  Inside the former the body is chosen per
 *     sample on the device: 1 <= popcount(valid[b] & mask(C)) <= 23 takes the sparse body, anything else the flat one.
 *   mt_multitalent_loss_bwd: "mt_loss_bwd_wide_kernel" (16-byte stores: cs == dcs == C >= 2, V * C % 4 == 0, both bases 16-byte
 *     aligned) | "mt_loss_bwd_flat_kernel" (cs == dcs == C) | "mt_loss_bwd_kernel".
 *   mt_softmax_dice_ce_fwd / _bwd (backward != 0): "softmax_loss_fwd_kernel<4>" (C <= 4), <8>, <16> | "softmax_loss_fwd_wide_kernel".
 * *vpb / *nblk (may be NULL): voxels per workgroup and workgroups per sample of the named kernel. */
int mt_multitalent_loss_fwd_kernel_name(int cs, long V, int C, char* buf, size_t n, long* vpb, int* nblk);
int mt_multitalent_loss_bwd_kernel_name(const float* logits, int cs, const float* dlogits, int dcs, long V, int C, char* buf, size_t n,
                                        long* vpb, int* nblk);
int mt_softmax_dice_ce_kernel_name(int C, int backward, char* buf, size_t n);

/* ---- optimizer (nnUNetTrainerV2.py:166-170; clip MultiTalent_Trainer_DDP.py:352,362) --------- */
int mt_sumsq(const float* x, long n, float* out /* [1], overwritten */, void* ws, size_t ws_bytes,
             mt_stream_t stream);
size_t mt_sumsq_workspace(long n);
/* torch.optim.SGD(nesterov=True, dampening=0): g = clip*g + wd*p; buf = mom*buf + g (buf=g on first
 * step); p -= lr*(g + mom*buf).  clip_coef_dev: device scalar total_norm^2 -> coef = min(1, max_norm/(sqrt+1e-6)) */
int mt_sgd_nesterov(float* p, const float* g, float* buf, long n, float lr, float wd, float mom,
                    int first_step, const float* sumsq_dev, float max_norm, mt_stream_t stream);

/* ---- sliding-window inference (neural_network.py:287-428,502-591) ---------------------------- */
/* acc[c][x] (+)= w * nonlin(logits[flip(x)][c])  NCDHW accumulator over one tile: mirror-TTA mean */
int mt_flip_accumulate(const float* logits, int cs, int D, int H, int W, int C, int flipD, int flipH,
                       int flipW, int nonlin /*0 none,1 sigmoid,2 softmax*/, float weight, float* acc,
                       int first, mt_stream_t stream);
/* Fused form of (1x1x1 head -> mt_flip_accumulate) for inference: p describes the head (src = its lazily activated input of N
 * samples, Cin, Cout <= 64, wpack layout 1 ck 16, bias; Db,Hb,Wb = tile size); sample `sample` is evaluated, passed through the
 * nonlinearity, un-flipped and accumulated into acc[Cout][D][H][W] like mt_flip_accumulate — the logits are never stored. */
int mt_head_flip_accumulate(const mt_pointwise_t* p, int sample, int flipD, int flipH, int flipW, int nonlin, float weight,
                            float* acc, int first, mt_stream_t stream);
/* All mirror combinations of one tile AND the overlap-add in one kernel: samples sample0 .. sample0+nsamples-1 of p's source are
 * the flipped versions of the tile (flips[k]: bit 0 D, bit 1 H, bit 2 W); per output voxel
 *   agg[c][x0+d][y0+h][z0+w] += gauss[d][h][w] * weight * sum_k nonlin(head(sample_k[flip_k(d,h,w)]))_c ;  nb[...] += gauss
 * (neural_network.py:531-586 and :384-394).  gauss NULL = 1, nb NULL = not updated.  flips is a HOST array of nsamples ints. */
int mt_head_mirror_accumulate(const mt_pointwise_t* p, int sample0, int nsamples, const int32_t* flips, int nonlin, float weight,
                              const float* gauss, float* agg, float* nb, long aX, long aY, long aZ, int x0, int y0, int z0,
                              mt_stream_t stream);
/* The kernel instance mt_head_flip_accumulate (mirror = 0) / mt_head_mirror_accumulate (mirror != 0) launches for p (profiler name,
 * e.g. "head_mirror_accumulate_kernel<2, 2>": elements per fp32 load — 1 dwords, 2 eight-byte pairs — and the source's storage type;
 * a 16-bit source is always <2, type>, one 16-byte load per lane).  It is decided from the source's storage type, channel stride and
 * base address by the function the launches call, and a head the launches refuse is refused here with the same code (sample range,
 * nonlinearity and the aggregate are not seen here).  Touches no device. */
int mt_head_infer_kernel_name(const mt_pointwise_t* p, int mirror, char* buf, size_t n);
/* The network batch of a group of tiles, mirror flips included, straight from the (padded) volume vol[C][X][Y][Z]:
 * out[k][C][D][H][W] = tile k at origin (x0,y0,z0) read through the reflections in `flips` (bit 0 D, bit 1 H, bit 2 W) —
 * `x = torch.flip(x, axes)` of neural_network.py:531-586 as index arithmetic.  desc: HOST array of ntiles x (x0, y0, z0, flips). */
int mt_extract_tiles(const float* vol, int C, long X, long Y, long Z, float* out, int ntiles, int D, int H, int W,
                     const int32_t* desc, mt_stream_t stream);
/* agg[c, tile] += acc * gauss ; nb[tile] += gauss   (neural_network.py:388-394) */
int mt_tile_accumulate(const float* acc, const float* gauss, int C, int D, int H, int W, float* agg,
                       float* nb, long aX, long aY, long aZ, int x0, int y0, int z0, mt_stream_t stream);
/* probs = agg/nb; seg = argmax_c or per-channel >0.5 in regions_class_order (neural_network.py:405-417) */
int mt_normalize_threshold(float* agg, const float* nb, int C, long V, const int32_t* class_order,
                           int use_regions, int32_t* seg, mt_stream_t stream);
/* Spatial augmentation (second half): batchgenerators' SpatialTransform as configured by
 * data_augmentation_moreDA.py:66-80 (rotation + scaling, order_data 3, order_seg 1, constant borders) = per sample
 * scipy.ndimage.map_coordinates over the affine field  x = M (o - (O-1)/2) + centre.
 * mt_spline_prefilter3: in-place cubic B-spline prefilter of vol[NC, D, H, W] (pole sqrt(3)-2, gain 6, scipy's exact mirror
 * boundary initialisation = what map_coordinates(order=3, mode='constant') filters with).
 * mt_affine_sample: dst[N, C, OD, OH, OW] from src[N, C, D, H, W]; mats = N x 12 floats (row-major 3x3 M, then the centre);
 * mode 0 nearest, 1 linear, 3 cubic (src must be prefiltered), 11 = segmentation rule for order 1 (label c where the linear
 * interpolation of (seg == c) is >= 0.5, larger labels override, else 0).  A coordinate outside [0, n-1] on any axis gives cval
 * (mode 11: 0); stencil taps off the array read the mirrored element (scipy 'constant' mode). */
int mt_spline_prefilter3(float* vol, int NC, int D, int H, int W, int axes /* bit 0 W, 1 H, 2 D; 7 = 3D, 3 = per slice */,
                         mt_stream_t stream);
int mt_affine_sample(const float* src, int N, int C, int D, int H, int W, float* dst, int OD, int OH, int OW,
                     const float* mats, int mode, float cval,
                     int planar /* 1: nnU-Net's "dummy 2D" augmentation — every D slice is an independent 2D image, OD == D */,
                     mt_stream_t stream);
/* Elastic deformation of the same transform (augment_spatial with do_elastic_deform; batchgenerators'
 * elastic_deform_coordinates): per mesh axis, offsets = gaussian_filter(uniform(-1, 1), sigma, mode='constant', cval=0) * alpha are
 * added to the zero-centred output mesh before rotation and scaling:  x = M (g(o) + alpha f(o)) + centre.
 * mt_gaussian_blur_axis_zero: ONE axis pass (0 D, 1 H, 2 W) of scipy.ndimage.gaussian_filter(mode='constant', cval=0, truncate=4)
 * over src[NC, D, H, W]: w[k] ~ exp(-k^2 / 2 sigma^2), k = -r..r, r = int(4 sigma + 0.5), weights and accumulation in double, taps
 * off the axis contribute 0 (no reflection), the result is rounded to float32.  sigma: HOST array of NC values, one per (sample,
 * channel); sigma <= 0 copies that channel.  A sigma whose radius exceeds 64 (sigma >= 16.125) or is NaN is refused with MT_EINVAL
 * before anything is launched — it is never clamped.  src != dst.
 * mt_warp_sample: mt_affine_sample with the displaced coordinate above.  field: [N, 3, OD, OH, OW] float32 (components d, h, w),
 * the element of an output voxel at that voxel's own index; planar: [N, 2, OH, OW] (components h, w), one field shared by all
 * slices, xd = od.  alpha: [N] device floats; for alpha[n] == 0 sample n's field is not read (it may be uninitialised) and the
 * result equals mt_affine_sample's bit for bit.  The displaced coordinate may lie anywhere or be non-finite: it is range-checked
 * in double before any integer conversion, and a NaN gives cval (mode 11: 0) like any coordinate outside the volume. */
int mt_gaussian_blur_axis_zero(const float* src, float* dst, int NC, int D, int H, int W, int axis,
                               const float* sigma /* [NC], host */, mt_stream_t stream);
int mt_warp_sample(const float* src, int N, int C, int D, int H, int W, float* dst, int OD, int OH, int OW,
                   const float* mats /* N x 12, as mt_affine_sample */,
                   const float* field /* [N, 3, OD, OH, OW]; planar: [N, 2, OH, OW] */,
                   const float* alpha /* [N] */, int mode /* 0, 1, 3, 11 */, float cval, int planar, mt_stream_t stream);
/* The resize unit (resize.hip, resize_line.h): resample_data_or_seg (preprocessing/preprocessing.py:109-197) at every order the
 * reference's preprocessors use.  skimage.transform.resize(order, mode='edge', anti_aliasing=False) is
 * scipy.ndimage.zoom(order, mode='nearest', grid_mode=True), the z pass is scipy.ndimage.map_coordinates(order_z, mode='nearest'):
 * output index o of an axis resized from `in` to `out` samples x = (o + 0.5) * in / out - 0.5 of the line extended by its edge values.
 * Volumes are [NC, D, H, W] float32; more than INT32_MAX input or output elements, a non-positive extent, a null pointer or an
 * order other than 0, 1, 3 is MT_EINVAL before any launch.
 * mt_resize_prefilter3: cubic B-spline prefilter (pole sqrt(3) - 2, gain 6) along the axes of the mask, src -> dst, src == dst
 *   allowed.  The edge rule needs no padded copy: c+[-1] = 6 x[0] / (1 - z) and
 *   c[n-1] = -(s z / (1 - z) + (c+[n-1] - s) z / (1 - z^2)), s = 6 x[n-1] / (1 - z).  Double recursion, one rounding to float32 per
 *   pass; a line of length 1 is copied.  With src != dst an axis that is not filtered is still copied by the first pass.
 * mt_resize: dst[NC, OD, OH, OW] with one order per axis.  An axis with in == out is copied whatever its order and must NOT be
 *   prefiltered; every other axis of order 3 must be.  Order 0: floor(x + 0.5) clamped; order 1: x clamped to [0, n - 1]; order 3: x
 *   is not clamped, taps floor(x) - 1 .. floor(x) + 2, and a tap at -2 .. -1 or n .. n + 1 is the coefficient of the extended line,
 *   c[-m] = x0 + (c[0] - x0) z^m with x0 = ((4 + z) c[0] + c[1]) / (5 + z) (mirrored at the end; n == 1: the value), folded into the
 *   weights of the two stored coefficients next to the edge.  Coordinates, weights and accumulation in double, output float32.
 *   A 3D resize gives one order on all axes; a per-slice resize leaves the anisotropic axis (any of the three) at in == out; the z pass
 *   changes one axis.  src != dst.
 * mt_resize_labels: batchgenerators' resize_segmentation(order 1) on the axes that change: the largest label whose order-1
 *   interpolated indicator is >= 0.5 (labels apply in ascending order), 0 where none is; -1 is a label like any other.
 * mt_resize_labels_axis: the z pass of a label map (preprocessing.py:176-184) along `axis` (0 D, 1 H, 2 W) to out_n: the same rule
 *   with the weight STRICTLY above 0.5 (np.round sends 0.5 to 0). */
int mt_resize_prefilter3(const float* src, float* dst, int NC, int D, int H, int W, int axes /* bit 0 W, 1 H, 2 D */, mt_stream_t stream);
int mt_resize(const float* src, int NC, int D, int H, int W, float* dst, int OD, int OH, int OW, int order_d, int order_h, int order_w,
              mt_stream_t stream);
int mt_resize_labels(const float* src, int NC, int D, int H, int W, float* dst, int OD, int OH, int OW, mt_stream_t stream);
int mt_resize_labels_axis(const float* src, int NC, int D, int H, int W, int axis, int out_n, float* dst, mt_stream_t stream);
/* Export post-processing: save_segmentation_nifti_from_softmax (segmentation_export.py:27-160) without the
 * resampled 47-channel intermediate — probabilities [C, D, H, W] are interpolated at the OD x OH x OW grid of the original
 * spacing (order 1, skimage/scipy half-pixel rule, edge clamp; sep_axis in 0..2 = the anisotropic axis sampled nearest as in
 * resample_data_or_seg's separate-z branch, preprocessing.py:134-187; -1 = trilinear), classified per voxel (use_regions: last
 * channel i in order with p_i > 0.5 gives class_order[i], else 0; otherwise argmax) and written as uint8 into the uncropped
 * volume out[FD, FH, FW] at offset (bD, bH, bW), clipped to the volume (crop_bbox re-insertion).  The caller zero-fills out. */
int mt_resample_classify(const float* probs, int C, int D, int H, int W, int OD, int OH, int OW, int sep_axis,
                         const int32_t* class_order, int use_regions, uint8_t* out, long FD, long FH, long FW,
                         int bD, int bH, int bW, mt_stream_t stream);
/* Ensemble merge (inference/ensemble_predictions.py:25-53 merge_files, evaluation/model_selection/ensemble.py:26-40 merge):
 * `np.mean(np.vstack([np.load(f)['softmax'][None] for f in files]), 0)` -> argmax, or the region thresholds in
 * regions_class_order -> re-insertion into the uncropped volume, in ONE streaming pass over the K members.
 * members: HOST array of K device pointers (1 <= K <= MT_ENSEMBLE_MAX_MEMBERS; they travel to the kernel by value), each to
 * float16 probabilities [C][chan_stride] of a D x H x W box, chan_stride >= V = D*H*W, 1 <= C <= 255.
 * Arithmetic = numpy's float16 mean, bit for bit: float32 accumulation in member order ((m0 + m1) + m2) + ..., ONE IEEE float32
 * division by (float)K, ONE round-to-nearest-even to float16, float16 subnormals kept.  The label is decided on that ROUNDED
 * float16 mean: argmax with the first maximum winning, or (use_regions) the last channel i with mean_i > 0.5 gives
 * class_order[i] (DEVICE int32[C], as in mt_resample_classify), else 0; the label is a uint8, so a class_order entry above 255
 * is stored as its low byte (entry & 255), the same on every store path.  A NaN mean follows numpy: np.argmax picks the first NaN
 * channel of a voxel, and a NaN mean is never > 0.5; the stored mean is numpy's.
 * out: uint8 [FD][FH][FW]; the box is written at offset (bD, bH, bW), which must lie inside the volume, clipped to the volume;
 * voxels outside the box are not touched.  mean: NULL, or float16 [C][mean_stride], mean_stride >= V (only the V voxels of each
 * channel are written).  Where the member pointers, mean, chan_stride and mean_stride are multiples of 8 elements every lane
 * moves 16 bytes; any other alignment (2-byte) is served element by element.
 * Traffic: 2*K*C*V bytes read, V written, + 2*C*V when the mean is kept. */
#define MT_ENSEMBLE_MAX_MEMBERS 16
int mt_ensemble_classify(const void* const* members, int K, int C, int D, int H, int W, long chan_stride,
                         const int32_t* class_order, int use_regions, uint8_t* out, long FD, long FH, long FW,
                         int bD, int bH, int bW, void* mean, long mean_stride, mt_stream_t stream);
/* Label-map file writer: gzip / DEFLATE encoding on the device (replaces `sitk.WriteImage` of a .nii.gz label map,
 * segmentation_export.py:148-160, and `gzip.open(..., compresslevel=1)` of utilities/nifti_io: raw voxels copied to the host and
 * compressed by one thread).  The uncompressed stream is prefix[0, n_prefix) — a HOST array of at most MT_DEFLATE_MAX_PREFIX bytes,
 * the 352 bytes of a NIfTI-1 header, so that the voxels are never copied or shifted on the device — followed by payload[0, n_payload)
 * on the DEVICE (uint8, any alignment).  It is cut into chunks of `chunk` bytes (MT_DEFLATE_MIN_CHUNK .. MT_DEFLATE_MAX_CHUNK; the
 * last may be shorter; an empty stream is one empty chunk) that are encoded independently, one workgroup each.
 * Tokens: every maximal run of equal bytes inside a chunk is its first byte as a literal, then matches of (distance 1, length 258)
 * while 258 bytes remain, then the remainder as one match when it is 3 or longer and as 1 or 2 literals otherwise; no match reaches
 * across a chunk boundary.  The token stream is a function of the bytes and `chunk` alone.
 * mt_deflate_tokenize: hist[0..285] = counts of the literal/length symbols of all chunks (one end-of-block per chunk included),
 *   hist[286..315] = counts of the distance symbols (only symbol 0 occurs); DEVICE uint32[316], zeroed by the call.  Each chunk's
 *   CRC-32 (IEEE) stays in the workspace for mt_deflate_emit.
 * mt_deflate_emit: the same stream, prefix, chunk and workspace after mt_deflate_tokenize, plus the code the HOST built from hist:
 *   table  HOST uint64[513]: a token's bits (first bit in bit 0, Huffman codes bit-reversed, extra bits behind their length code, the
 *          distance code behind those) in bits 0..47 and their number in bits 48..63; entry b = literal b, 256 + (L - 3) = match of
 *          length L, 512 = end of block;
 *   header HOST uint32 words, header_bits bits: the dynamic block's header behind its BFINAL bit (BTYPE, HLIT, HDIST, HCLEN, the
 *          code-length code, the coded lengths), unused high bits zero.
 *   A chunk becomes one dynamic block: BFINAL (set in the last chunk only), header, tokens, end of block; every chunk but the last
 *   is then byte-aligned by an empty stored block (3 zero bits, padding, 00 00 ff ff).  Where stored blocks (of up to 65535 bytes)
 *   are smaller than that, the chunk is written as stored blocks instead, which end byte-aligned by themselves.  The raw DEFLATE
 *   stream is the concatenation of the chunks.
 *   out (DEVICE, 8-byte aligned, mt_deflate_bound bytes): int64 total, uint32 crc[nchunks], padding to 8 bytes, then the `total`
 *   bytes of the DEFLATE stream.  The gzip framing (10-byte header, CRC-32 joined from the chunk CRCs, ISIZE) is the host's.
 * mt_deflate_workspace / mt_deflate_bound: bytes of ws (16-byte aligned, caller-owned, no content expected) and of out for a
 *   stream of n = n_prefix + n_payload bytes; both cover every chunk being stored; 0 for arguments the entry points refuse.
 * Errors: n > INT32_MAX, a chunk or prefix size outside the limits, a token of more than 48 bits are MT_EINVAL, a short ws is
 *   MT_EWORKSPACE, all before any launch.  Bits are written with integer atomic OR into zeroed words, tokens own disjoint bit
 *   ranges: the output is bit-identical from run to run.  Nothing is synchronised. */
#define MT_DEFLATE_MAX_PREFIX 512
#define MT_DEFLATE_MIN_CHUNK 32
#define MT_DEFLATE_MAX_CHUNK (1 << 24)
size_t mt_deflate_workspace(long n, int chunk);
size_t mt_deflate_bound(long n, int chunk);
int mt_deflate_tokenize(const uint8_t* payload, long n_payload, const uint8_t* prefix /* host */, int n_prefix, int chunk,
                        void* ws, size_t ws_bytes, uint32_t* hist /* device, 316 */, mt_stream_t stream);
int mt_deflate_emit(const uint8_t* payload, long n_payload, const uint8_t* prefix /* host */, int n_prefix, int chunk,
                    const uint64_t* table /* host, 513 */, const uint32_t* header /* host */, int header_bits,
                    void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes, mt_stream_t stream);
/* The same encoder for payloads of multi-byte elements (stored float16 probabilities and float32 training cases in .npz members,
 * where the reference calls np.savez_compressed) and for streams of more than one call.  Two more arguments:
 * period (1, 2, 4 or 8; anything else is MT_EINVAL before any launch): position p of a chunk is IN A RUN when p - period lies in
 *   the same chunk and byte[p] == byte[p - period].  A maximal stretch of L such positions is matches of (distance period, length
 *   258) while 258 positions remain, then the remainder as one match when it is 3 or longer and as 1 or 2 literals otherwise; every
 *   other position is a literal.  (Matches longer than their distance overlap, which DEFLATE allows.)  period 1 is the token stream
 *   above.  The distance counter that is used is hist[286 + period - 1] for periods 1, 2 and 4 and hist[286 + 5] for period 8
 *   (distance code 5 covers 7..8 with one extra bit, which the host puts into the table's match entries).
 * final: 0 leaves BFINAL clear in the last chunk and byte-aligns it with the empty stored block like every other chunk, so that
 *   the outputs of consecutive calls concatenate into one DEFLATE stream (each call with its own code table; the host joins the
 *   CRCs).  That is how a member of more than INT32_MAX bytes is written.
 * mt_deflate_tokenize / mt_deflate_emit are these with period = 1 and final = 1.  A lane packs its consecutive tokens in registers
 * and stores whole words; only the first and last word of its bit range are shared with its neighbours and written with atomic OR. */
int mt_deflate_tokenize_period(const uint8_t* payload, long n_payload, const uint8_t* prefix /* host */, int n_prefix, int chunk,
                               int period, void* ws, size_t ws_bytes, uint32_t* hist /* device, 316 */, mt_stream_t stream);
int mt_deflate_emit_period(const uint8_t* payload, long n_payload, const uint8_t* prefix /* host */, int n_prefix, int chunk,
                           int period, int final, const uint64_t* table /* host, 513 */, const uint32_t* header /* host */,
                           int header_bits, void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes, mt_stream_t stream);
/* Reader of the same files: INFLATE (RFC 1951: stored, fixed and dynamic blocks, every length and distance code) of a raw DEFLATE
 * stream comp[0, n_comp) in DEVICE memory (any alignment, 1 .. INT32_MAX - 64 bytes), parallel over the stream's byte-aligned
 * restart points.  A UNIT starts at a byte position, decodes consecutive blocks and ends behind an EMPTY stored block (3 bits,
 * padding, 00 00 ff ff: what mt_deflate_emit puts behind every Huffman-coded chunk and zlib's Z_FULL_FLUSH behind its data; the
 * next unit starts at the following byte) or at a block with BFINAL.  Non-empty stored blocks belong to the unit they occur in.
 * mt_inflate_scan: candidates are position 0 and every position behind an occurrence of 00 00 ff ff, in order; more than
 *   n_comp / 5 + 2 of them (true units are at least 5 bytes long) is status FOREIGN.  Every candidate is decoded without output by
 *   one wave: a read behind the input, an invalid block, an over-subscribed code, an unassigned code or a match that reaches in
 *   front of its unit make it BAD, more than unit_limit (1 .. 2^30) bytes from Huffman-coded blocks TOO_LONG.  One wave then
 *   follows end -> start from position 0: every end must be a candidate; a candidate on the way that failed gives its status to the
 *   stream, an end that is no candidate, or a chain that does not end at n_comp with BFINAL (final != 0) / at n_comp with or
 *   without it (final == 0: the body of mt_deflate_emit_period with final = 0), gives CORRUPT.  Candidates that are not reached
 *   are ignored, whatever they decoded to.  n_expect >= 0 and a different total gives SIZE.
 *   ws (DEVICE, 16-byte aligned, mt_inflate_workspace(n_comp) bytes) begins with { int32 status; int32 n_units; int64 total;
 *   int32 n_cand; int32 n_spans; }: status 0 OK, 1 FOREIGN, 2 TOO_LONG, 3 BAD, 4 CORRUPT, 5 SIZE; behind it the candidates,
 *   their results and the chain (start, output offset as a 64-bit exclusive scan, stored blocks) for mt_inflate_write.
 * mt_inflate_write: the same comp and ws after a scan with status OK, its n_units, n_spans and n_out == total.  The non-empty
 *   stored blocks of the chained units are listed and copied by the whole grid, then one wave per unit decodes again into its own
 *   range out[offset, offset + bytes) and nowhere else (the values are checked against the head on the device: a mismatch writes
 *   nothing).  The output is staged in LDS and leaves in 16-byte stores; matches nearer than 3838 bytes are served from LDS.
 * mt_inflate_crc: crcs[k] (DEVICE) = CRC-32 of data[k * piece, min(n, (k + 1) * piece)), piece 16 .. 2^24; one entry for n == 0.
 * Errors: sizes outside these limits, a NULL or misaligned argument are MT_EINVAL, a short ws MT_EWORKSPACE, all before any
 *   launch; what the stream holds is reported through the status, never through the return value.  Nothing is synchronised. */
size_t mt_inflate_workspace(long n_comp);
/* where the workspace keeps what a caller may want to look at after a scan: part 0 = byte offset of the candidate positions
 * (int32, ascending), 1 = byte offset of the chain (int32 index into the candidates, one per unit), 2 = entries of either table;
 * 0 for other arguments. */
size_t mt_inflate_workspace_part(long n_comp, int part);
int mt_inflate_scan(const uint8_t* comp, long n_comp, long unit_limit, int final, long n_expect, void* ws, size_t ws_bytes,
                    mt_stream_t stream);
int mt_inflate_write(const uint8_t* comp, long n_comp, void* ws, size_t ws_bytes, int n_units, int n_spans, uint8_t* out,
                     long n_out, mt_stream_t stream);
int mt_inflate_crc(const uint8_t* data, long n, int piece, uint32_t* crcs, mt_stream_t stream);
/* INFLATE of a raw DEFLATE stream WITHOUT restart points (a file of another writer: zlib, numpy, gzip, pigz), parallel over block
 * starts that are found by search (csrc/inflate_spec.hip).  comp[0, n_comp) in DEVICE memory, any alignment, 1 ..
 * INT32_MAX - 64 bytes; chunk: a power of two in 64 .. 2^20.  Positions are BIT positions (64-bit).  A UNIT starts at a candidate,
 * decodes consecutive blocks and ends at the first block end that is a candidate's position, or at a block with BFINAL (the stream
 * ends at the next byte boundary).  Its matches may reach up to 32768 bytes in front of it.
 * mt_inflate_spec_scan: candidates are bit 0 and, for every chunk of `chunk` compressed bytes, the first bit position p > 0 in the
 *   chunk at which the header of a non-final dynamic block is accepted as zlib's inflate accepts one (HLIT <= 29, HDIST <= 29, a
 *   complete code-length code, a valid length sequence with a length for symbol 256, neither code over-subscribed and each complete
 *   unless its longest code is one bit, no header bit behind the input); the header may extend past the chunk.  Every candidate is
 *   decoded without output by one wave: more than unit_limit (1 .. 2^30) output bytes or more than span_limit (>= 1) consumed
 *   compressed bytes is TOO_LONG, an invalid block or code or a read behind the input BAD, a match in front of bit 0 CORRUPT.  One
 *   wave then follows end -> start from bit 0: a candidate on the way that failed gives the stream its status, a last unit without
 *   BFINAL or one that does not end at n_comp CORRUPT, n_expect >= 0 and another total SIZE.  Candidates that are not reached
 *   are ignored, so the result never depends on what the search accepts.  steps: a mask of 1 search, 2 size pass, 4 chain (7: all;
 *   the parts exist so that a caller can time them, each needs the ones in front of it in the same ws).
 *   ws (DEVICE, 16-byte aligned, mt_inflate_spec_workspace(n_comp, chunk) bytes: 60 per chunk) begins with { int32 status; int32
 *   n_units; int64 total; int32 n_cand; int32 n_spans; int32 max_reach; uint32 shortest_unit; }: the statuses of mt_inflate_scan;
 *   max_reach = the farthest a match of a chained unit reaches in front of its unit, shortest_unit = the fewest bytes of one.
 *   mt_inflate_spec_workspace_part: part 0 = byte offset of the candidates' bit positions (int64, ascending), 1 = byte offset of
 *   the chain (int32 index into the candidates, one per unit), 2 = entries of either table; 0 for other arguments.
 * mt_inflate_spec_write: the same comp, chunk and ws after a scan with status OK, its n_units, n_spans and n_out == total, and ws2
 *   (DEVICE, 16-byte aligned, mt_inflate_spec_write_workspace(n_units, n_spans, n_out) bytes: 2 per output byte, 32768 per unit,
 *   16 per stored block).  steps: a mask of 1 symbols (the non-empty stored blocks are copied by the whole grid, then one wave per
 *   unit decodes into 16-bit symbols: a byte, or 0x8000 | index into the 32768 bytes in front of the unit), 2 windows (one
 *   workgroup resolves every unit's last 32768 bytes in order), 4 resolve (out[i] from its symbol and the window in front of its
 *   unit, 16-byte stores).  A marker that points in front of the stream sets the head's status to CORRUPT, which the caller reads
 *   after the call; out then holds zeros there.  The values are checked against the head on the device: a mismatch writes nothing.
 * Errors as for mt_inflate_*: MT_EINVAL / MT_EWORKSPACE before any launch, the stream's verdict is a status.  Nothing is
 *   synchronised, there is no process-wide state. */
size_t mt_inflate_spec_workspace(long n_comp, int chunk);
size_t mt_inflate_spec_workspace_part(long n_comp, int chunk, int part);
size_t mt_inflate_spec_write_workspace(int n_units, int n_spans, long n_out);
int mt_inflate_spec_scan(const uint8_t* comp, long n_comp, int chunk, long unit_limit, long span_limit, long n_expect, int steps,
                         void* ws, size_t ws_bytes, mt_stream_t stream);
int mt_inflate_spec_write(const uint8_t* comp, long n_comp, int chunk, void* ws, size_t ws_bytes, int n_units, int n_spans, void* ws2,
                          size_t ws2_bytes, uint8_t* out, long n_out, int steps, mt_stream_t stream);
/* Connected-component post-processing (remove_all_but_the_largest_connected_component, postprocessing/connected_components.py:48-101).
 * mt_cc_label3d: `lmap, num_objects = scipy.ndimage.label(mask)` (:76) with scipy's default 3-D structure, 6-connectivity (face
 * neighbours only), on the mask {v : member[seg[v]] != 0} of a contiguous uint8 volume seg[D, H, W].  member: HOST array of 256
 * entries (a tuple entry such as (1, 2) of for_which_classes is one joint mask).  Outputs, caller-allocated device arrays of
 * V = D*H*W int32:
 *   labels[v] = the smallest linear index (d*H + h)*W + w of v's component, -1 for background — a function of the partition alone,
 *               bit-identical from run to run whatever the scheduling;
 *   sizes[v]  = the component's exact voxel count where v is that smallest index (labels[v] == v), 0 everywhere else;
 *   stats[0]  = number of components, stats[1] = largest count (0 when the mask is empty); device int32[2].
 * mt_cc_remove: the removal loop (:85-100) in place on seg, for the labelling above: a component with count c is zeroed when
 *   (double)c * volume_per_voxel != (double)stats[1] * volume_per_voxel   (every component tied for the largest is kept, `!= maximum_size`)
 * and, when use_min_size != 0, (double)c * volume_per_voxel < min_size — evaluated in fp64 on the device, the same IEEE product as the
 * reference's np.int64 * float.  *removed (device int32) = the largest removed count, 0 when nothing was removed; the host forms
 * largest_removed = removed * volume_per_voxel and kept_size = stats[1] * volume_per_voxel as the reference does.
 * Both reject V > INT32_MAX with MT_EINVAL before any launch. */
int mt_cc_label3d(const uint8_t* seg, int D, int H, int W, const uint8_t* member, int32_t* labels, int32_t* sizes, int32_t* stats,
                  mt_stream_t stream);
int mt_cc_remove(uint8_t* seg, int D, int H, int W, const int32_t* labels, const int32_t* sizes, const int32_t* stats,
                 double volume_per_voxel, int use_min_size, double min_size, int32_t* removed, mt_stream_t stream);
/* Cropping a case to its non-zero region (preprocessing/cropping.py:23-116; preprocessing/device_cropping.py).
 * mt_nonzero_mask: mask[v] = 1 when any of the C channels of the contiguous float32 data[C][V] is != 0 at v, else 0 (:23-29 before
 *   the hole filling).  Numpy's rule, decided on the bit pattern ((bits & 0x7fffffff) != 0): NaN, +-inf and denormals are non-zero,
 *   -0.0 is zero, whatever the denormal mode.  Any V, any alignment of mask (data: 4 bytes).
 * mt_fill_holes3d: in place on the contiguous uint8 volume mask[D, H, W]:  mask = scipy.ndimage.binary_fill_holes(mask != 0)  with
 *   scipy's default structure (face neighbours only), values 0 / 1: the 6-connected components of the background are labelled with
 *   the launches of mt_cc_label3d, and a component is filled exactly when none of its voxels lies on a face of the volume (with an
 *   axis of length 1 every voxel does, and nothing is filled).  bbox: device int32[7] = lo_d, hi_d, lo_h, hi_h, lo_w, hi_w of the
 *   result (hi exclusive, get_bbox_from_mask's convention) and its number of set voxels; a count of 0 means an empty mask, the box
 *   is then unspecified.  Integer atomics only: mask and bbox are bit-identical from run to run.
 *   ws: mt_fill_holes3d_workspace(D, H, W) bytes of device scratch, 16-byte aligned (4 bytes per voxel + 16); too small a workspace
 *   is MT_EWORKSPACE, D*H*W > INT32_MAX is MT_EINVAL, both before any launch.
 * mt_crop_nonzero: one pass over the HOST box[6] = lo_d, hi_d, lo_h, hi_h, lo_w, hi_w:  out[c] = data[c][box] bit for bit (C channels,
 *   NaN payloads included), and the segmentation of :98-115.  seg_in == NULL: seg_out is int8 [1][box], 0 inside the mask and
 *   nonzero_label (an int8 value) outside.  Otherwise seg_in is float32 [CS][D, H, W] and seg_out float32 [CS][box]:
 *   seg_out[c] = nonzero_label where seg_in[c] == 0 and mask == 0, else seg_in[c].  D*H*W > INT32_MAX is MT_EINVAL. */
int mt_nonzero_mask(const float* data, int C, long V, uint8_t* mask, mt_stream_t stream);
size_t mt_fill_holes3d_workspace(int D, int H, int W);
int mt_fill_holes3d(uint8_t* mask, int D, int H, int W, int32_t* bbox, void* ws, size_t ws_bytes, mt_stream_t stream);
int mt_crop_nonzero(const float* data, int C, int D, int H, int W, const uint8_t* mask, const int32_t* box /* host, 6 */, float* out,
                    const float* seg_in /* NULL or [CS][D, H, W] */, int CS, void* seg_out, float nonzero_label, mt_stream_t stream);
/* Preprocessing a training case (preprocessing/preprocessing.py:273-353; preprocessing/device_preprocessing.py).  Additions to ABI 4.
 * mt_masked_moments: for each of the C channels of the contiguous float32 data[C][V], over the voxels a predicate selects:
 *   stats[c] (device doubles) = count, mean, population standard deviation (numpy's std, ddof 0).  Predicates: MT_MOMENTS_ALL,
 *   MT_MOMENTS_SEG_GE0 (seg[v] >= 0, seg: float32 [V] shared by the channels), MT_MOMENTS_OPEN_RANGE (lo[c] < x < hi[c], HOST doubles,
 *   compared in double).  Two passes in double (the mean, then the centred squares); per-block partials are combined in a fixed
 *   order by a second small launch, no floating-point atomics: bit-identical from run to run.  An empty selection gives count 0 and
 *   NaN for mean and sd.  At most 16 channels.  ws: mt_masked_moments_workspace(C, V) bytes of device scratch, 8-byte aligned.
 * mt_intensity_normalize: in place on one channel x[V]:  x = clip(x, lo, hi) when clip != 0, then x = (x - m) / (s + eps) in float32
 *   with a true division (numpy's arithmetic order), where (m, s) = (mean, sd), or (float)stats[1], (float)stats[2] of a device
 *   triple that mt_masked_moments wrote when stats != NULL.  The clip is np.clip's two comparisons: a NaN voxel passes it and stays
 *   NaN.  seg != NULL: voxels with seg[v] < 0 become 0, the reference's `data[seg < 0] = 0` after normalising; its other masked form,
 *   `mask = seg >= 0; data[mask] = ...; data[mask == 0] = 0`, gives the same result for every seg but a NaN one, which `seg < 0`
 *   leaves normalised and `mask == 0` would zero (a label map holds no NaN; the kernel follows `seg < 0`).
 * mt_label_counts / mt_label_locations: the class locations of _run_internal (:340-351).  seg: float32 label map [V]; a voxel belongs
 *   to slot table[(int)seg[v]] when seg[v] is an integer in 0..L-1 and that entry is < nslots (table: L device bytes, 255 = no slot;
 *   nslots <= 255).  mt_label_counts: counts[slot] (device int64) = number of voxels of the slot; it also leaves, in ws, the
 *   exclusive offsets of every (slot, unit of MT_PP_UNIT consecutive voxels), which mt_label_locations needs: same seg, table, ws.
 *   mt_label_locations: out[i] (device int64 [nq][3]) = the [x, y, z] coordinate in the [D, H, W] volume of the qrank[i]-th voxel
 *   (C order, 0-based) of slot qslot[i], i.e. np.argwhere(seg == c)[rank]; a query outside the counts gives -1, -1, -1.  An ordered
 *   compaction (unit counts, scan, int32 linear indices into idx, gather): the result does not depend on block scheduling.
 *   idx: device int32 scratch of idx_capacity >= sum(counts) entries.  ws: mt_label_counts_workspace(V, nslots) bytes, 8-byte
 *   aligned.  V > INT32_MAX is MT_EINVAL before any launch. */
#define MT_MOMENTS_ALL 0
#define MT_MOMENTS_SEG_GE0 1
#define MT_MOMENTS_OPEN_RANGE 2
#define MT_PP_UNIT 8192
size_t mt_masked_moments_workspace(int C, long V);
int mt_masked_moments(const float* data, int C, long V, int pred, const float* seg, const double* lo /* host, C */,
                      const double* hi /* host, C */, double* stats, void* ws, size_t ws_bytes, mt_stream_t stream);
int mt_intensity_normalize(float* x, long V, int clip, float lo, float hi, float mean, float sd, const double* stats, float eps,
                           const float* seg, mt_stream_t stream);
size_t mt_label_counts_workspace(long V, int nslots);
int mt_label_counts(const float* seg, long V, const uint8_t* table, int L, int nslots, int64_t* counts, void* ws, size_t ws_bytes,
                    mt_stream_t stream);
int mt_label_locations(const float* seg, int D, int H, int W, const uint8_t* table, int L, int nslots, void* ws, size_t ws_bytes,
                       int32_t* idx, long idx_capacity, const int32_t* qslot, const int64_t* qrank, long nq, int64_t* out,
                       mt_stream_t stream);
/* Intensity augmentation of the training chain (data_augmentation_moreDA.py:90-106: BrightnessMultiplicativeTransform,
 * ContrastAugmentationTransform, the inverted and the plain GammaTransform; training/data_augmentation/color.py).  Additions to ABI 4.
 * Both calls work on a contiguous float32 batch x[NC][V] (the [N, C, D, H, W] batch, NC = N*C, every channel volume contiguous;
 * with NC = N, V = C*V the same calls treat a whole sample as one channel).  Nothing is read back: the statistics stay in device
 * memory, the parameters drawn on the host travel in the kernel arguments.  V > INT32_MAX is MT_EINVAL before any launch.
 * mt_channel_stats: for every channel c with active[c] != 0 (HOST bytes, NC of them; NULL = all)
 *   stats[c] (device doubles, [NC][4]) = min, max, mean, population standard deviation (ddof 0) of x[c].  An inactive channel is not
 *   read and its row of stats is not written.  Min and max are exact.  ONE pass over the data (4 bytes per element), all channels in
 *   one launch: the sums are those of the SHIFTED values d = x - x[c][0], sum(d) and sum(d*d) in double, mean = x[c][0] + sum(d)/V,
 *   variance = (sum(d*d) - sum(d)^2/V)/V.  The shift is a sample of the channel, so (shift - mean)^2 <= V * variance and the
 *   subtraction loses at most log2(V) <= 31 of the 53 bits: a channel whose mean is 100 times (or 10^6 times) its sd keeps its sd.
 *   Per-workgroup partials are combined in a fixed order by a second small launch, no floating-point atomics: bit-identical from
 *   run to run.  A constant channel gives sd 0 exactly.  Non-finite elements follow numpy: a channel that holds a NaN has NaN for
 *   all four statistics; one that holds an infinity (and no NaN) has its exact min and max, numpy's mean (+-inf, NaN with both signs)
 *   and a NaN sd.  (The shift is 0 when x[c][0] is not finite.)
 *   ws: mt_channel_stats_workspace(NC, V) bytes of device scratch, 8-byte aligned; a smaller one is MT_EINVAL before any launch.
 * mt_intensity_apply: in place, one launch per 64 channels.  records: HOST array of NC mt_intensity_op_t, one per channel:
 *   MT_INTENSITY_NONE      the channel is neither read nor written;
 *   MT_INTENSITY_SCALE     x *= a                                                    (brightness, :90; needs no statistics)
 *   MT_INTENSITY_CONTRAST  x = (x - mean) * a + mean, then clamped to [min, max] when flags has MT_INTENSITY_PRESERVE_RANGE    (:91)
 *   MT_INTENSITY_GAMMA     with y = -x when flags has MT_INTENSITY_NEGATE (invert_image, :104), else x, and min / max of y derived
 *                          from those of x (min <-> -max):  y = ((y - min) / (max - min + b))^a * (max - min) + min,  b = epsilon;
 *                          -y is stored when negated                                                                (:104-106)
 *   MT_INTENSITY_RESTORE   retain_stats of the same transforms: y = (y - mean1) / (sd1 + 1e-8) * sd0 + mean0 in the same (negated)
 *                          domain, (mean0, sd0) from stats[c] (taken before the gamma), (mean1, sd1) from stats2[c] (taken after it).
 *   stats, stats2: device arrays of mt_channel_stats written earlier on the same stream (NULL where no record needs them: SCALE and
 *   NONE need none, only RESTORE needs stats2).  All arithmetic is float32 in the order written, every operation rounded on its own,
 *   true divisions; the statistics are rounded to float32 once.  A constant channel (range 0, sd 0) gives what the formulas give,
 *   finite values; the base of the power is >= 0 by construction and 0^a = 0.  The op is uniform per workgroup, so a launch that mixes
 *   ops does not make the scaled channels pay for the power.  An unknown op, or a record whose statistics are NULL, is MT_EINVAL
 *   before any launch. */
#define MT_INTENSITY_NONE 0
#define MT_INTENSITY_SCALE 1
#define MT_INTENSITY_CONTRAST 2
#define MT_INTENSITY_GAMMA 3
#define MT_INTENSITY_RESTORE 4
#define MT_INTENSITY_PRESERVE_RANGE 1
#define MT_INTENSITY_NEGATE 2
typedef struct { int32_t op, flags; float a, b; } mt_intensity_op_t;
size_t mt_channel_stats_workspace(int NC, long V);
int mt_channel_stats(const float* x, int NC, long V, const uint8_t* active /* host, NC, or NULL */, double* stats /* [NC][4] */,
                     void* ws, size_t ws_bytes, mt_stream_t stream);
int mt_intensity_apply(float* x, int NC, long V, const mt_intensity_op_t* records /* host, NC */, const double* stats,
                       const double* stats2, mt_stream_t stream);
/* Evaluation (evaluation/evaluator.py, evaluation/metrics.py:314-383).
 * mt_seg_joint_hist: one pass over two contiguous uint8 label volumes of V voxels (any alignment; V is not limited to int32):
 *   hist[remap[test[v]] * C + remap[ref[v]]] += 1, exact 64-bit counts in the device array hist[C * C] (zeroed by the call).
 *   remap: HOST array of 256 entries, every one below C (1..256).  The confusion counts of a label entry - an int or a tuple such
 *   as (1, 2) - are sums of cells, so all entries of a case cost one launch.  C <= 64 counts in workgroup-private LDS bins,
 *   larger C with global atomics; integer sums: the result does not depend on the scheduling.
 * mt_surface_distances: medpy's __surface_distances in both directions for the masks {v : member[test[v]]} (A) and
 *   {v : member[ref[v]]} (B) of two contiguous uint8 volumes [D, H, W]; member: HOST array of 256 entries.
 *     border(X) = X ^ binary_erosion(X, generate_binary_structure(3, connectivity)), border_value 0 (a mask voxel on a volume
 *                 face is a border voxel), connectivity 1..3;
 *     sds(A->B) = distance_transform_edt(~border(B), sampling = spacing)[border(A)]: for every border voxel of A, in linear
 *                 index order, sqrt((dz sz)^2 + (dy sy)^2 + (dx sx)^2) in fp64 of the integer offsets to a nearest border voxel
 *                 of B (exact: the nearest site is searched over all candidates in fp64); +inf when B has no border voxel.
 *   spacing: HOST (z, y, x) doubles, NULL = (1, 1, 1).  out: device array of `capacity` doubles: sds(A->B) at [0, nA), sds(B->A)
 *   at [nA, nA + nB); entries at or beyond `capacity` are dropped (the number of mask voxels |A| + |B| always suffices).
 *   stats: device double[6] = (nA, max, sum) of A->B, then (nB, max, sum) of B->A; the counts are the true ones, so
 *   nA + nB > capacity tells the caller that `out` and the maxima / sums are truncated.  Sums are formed in a fixed order without
 *   floating-point atomics: `out` and `stats` are bit-identical from run to run.
 *   ws: mt_surface_distances_workspace(D, H, W, capacity) bytes of device scratch, 16-byte aligned (5 bytes per voxel and
 *   4 per entry of capacity).  D*H*W > INT32_MAX, or an axis above 32766, is rejected with MT_EINVAL before any launch.
 * mt_select_kth: out[r] (device doubles) = the ranks[r]-th smallest (0-based) of the n doubles x (8-byte aligned; any n >= 1: the
 *   former limit of 2^32 - 1 elements is gone), for nranks <= 8 HOST ranks: the float64 width of the radix select of mt_select_kth_f32
 *   below, 8 passes of 8 bits on the key bits ^ (sign ? all ones : sign bit).  The key orders doubles of either sign (-0.0 before
 *   +0.0, NaNs by bit pattern); among the non-negative doubles the entry point was first specified for it selects exactly the element
 *   the plain bit pattern selects.  ws: mt_select_kth_workspace(nranks) bytes of device scratch, 8-byte aligned: ask every time, the
 *   size is not that of earlier builds.  n < 1, a rank outside 0..n-1 or nranks outside 1..8 is MT_EINVAL, too small a workspace
 *   MT_EWORKSPACE, both before any launch.
 * mt_sd_count_within (an addition to ABI 4): counts[s * T + t] (device int64[2][T], 8-byte aligned) = the number of distances
 *   <= tols[t] in segment s of the array mt_surface_distances wrote: segment 0 = sds[0, n_tr), segment 1 = sds[n_tr, n_tr + n_rt).
 *   The normalized surface Dice of evaluation/surface_dice.py:43-56 is host arithmetic on these integers.  tols: HOST array of T
 *   (1..8) doubles, passed to the kernel by value; the comparison is fp64, so a distance equal to the tolerance is within it; +inf
 *   counts everything (a NaN distance is within nothing).  The call zeroes `counts` on the stream before the launch: the caller need
 *   not.  One pass, 8 bytes read per distance; 16-byte loads where the address allows (sds needs 8-byte alignment only and
 *   n_tr may be odd).  One 64-bit integer atomic per workgroup, segment and tolerance, nothing else: identical from run to run.  T outside 1..8, a negative segment length, n_tr + n_rt < 1,
 *   a NaN or negative tolerance, a null or misaligned pointer is MT_EINVAL before any launch. */
int mt_sd_count_within(const double* sds, long n_tr, long n_rt, const double* tols /* host */, int T, int64_t* counts, mt_stream_t stream);
int mt_seg_joint_hist(const uint8_t* test, const uint8_t* ref, long V, const uint8_t* remap, int C, int64_t* hist, mt_stream_t stream);
size_t mt_surface_distances_workspace(int D, int H, int W, long capacity);
int mt_surface_distances(const uint8_t* test, const uint8_t* ref, int D, int H, int W, const uint8_t* member, const double* spacing,
                         int connectivity, double* out, long capacity, double* stats, void* ws, size_t ws_bytes, mt_stream_t stream);
size_t mt_select_kth_workspace(int nranks);
int mt_select_kth(const double* x, long n, const long* ranks, int nranks, double* out, void* ws, size_t ws_bytes, mt_stream_t stream);
/* The dataset fingerprint (experiment_planning/DatasetAnalyzer.py:161-224; multitalent_amd/experiment_planning/DatasetAnalyzer.py) and
 * the np.unique of a label map (preprocessing/cropping.py:146, DatasetAnalyzer.py:83).  Additions to ABI 4.
 * mt_fg_sample_count / mt_fg_sample_gather: data[c][seg > 0][::stride] for the C channels of the contiguous float32 data[C][V] at once.
 *   The selection is the voxels with seg[v] > 0 (seg: float32 [V]; a float comparison: -1, 0 and NaN are not selected); n = their
 *   number, m = ceil(n / stride).  mt_fg_sample_count: *count (device int64) = n; it also leaves, in ws, the exclusive offset of
 *   every unit of MT_PP_UNIT consecutive voxels, which mt_fg_sample_gather needs: same seg, ws.  mt_fg_sample_gather:
 *   out[c * out_cs + j] = data[c][v_(j * stride)] for j < m, where v_r is the r-th selected voxel in C order: bit for bit, NaN
 *   payloads included; nan_counts[c] (device int64) = the number of NaNs among channel c's m samples.  out_cs >= m is the channel
 *   stride of out (a case can be written into its slot of a larger buffer); samples at or beyond out_cs are dropped.  An ordered
 *   compaction (unit counts, scan, ballot ranks) with integer arithmetic only: the result does not depend on block scheduling.
 *   ws: mt_fg_sample_workspace(V) bytes of device scratch, 8-byte aligned.  V > INT32_MAX, C > 16 or stride < 1 is MT_EINVAL, too
 *   small a workspace MT_EWORKSPACE, both before any launch.
 * mt_select_kth_f32: out[r] (device float32) = the ranks[r]-th smallest (0-based) of the n float32 values x (4-byte aligned; n may
 *   exceed 2^32), for nranks <= 8 HOST ranks: radix select, 4 passes of 8 bits, on the key bits ^ (sign ? 0xffffffff : 0x80000000).
 *   The result is an element of x: -0.0 orders before +0.0, +-inf and denormals order as numbers, NaNs by bit pattern (the result
 *   is then unspecified).  All ranks share each pass over x; integer histograms: bit-identical from run to run.
 *   ws: mt_select_kth_f32_workspace(nranks) bytes of device scratch, 8-byte aligned.  n < 1, a rank outside 0..n-1 or nranks
 *   outside 1..8 is MT_EINVAL, too small a workspace MT_EWORKSPACE, both before any launch.
 * mt_label_presence: one pass over the float32 label map seg[V] (any V): bit (l + 1) % 32 of bitmap[(l + 1) / 32] (device uint32[32])
 *   is set exactly when some voxel equals the integer l in -1..1022; *flag (device int32) = 1 when any voxel is non-integral, NaN or
 *   outside that range, else 0.  Both are written by the call (no need to clear them). */
size_t mt_fg_sample_workspace(long V);
int mt_fg_sample_count(const float* seg, long V, int64_t* count, void* ws, size_t ws_bytes, mt_stream_t stream);
int mt_fg_sample_gather(const float* data, int C, long V, const float* seg, long stride, const void* ws, size_t ws_bytes, float* out,
                        long out_cs, int64_t* nan_counts, mt_stream_t stream);
size_t mt_select_kth_f32_workspace(int nranks);
int mt_select_kth_f32(const float* x, long n, const long* ranks /* host */, int nranks, float* out, void* ws, size_t ws_bytes,
                      mt_stream_t stream);
int mt_label_presence(const float* seg, long V, uint32_t* bitmap, int32_t* flag, mt_stream_t stream);
/* The dataset conversion (dataset_conversion/Task100_MultiTalent.py:229-275, copy_and_convert_segmentation; multitalent_amd/
 * dataset_conversion/Task100_MultiTalent.py).  Additions to ABI 4.
 * mt_label_convert: one pass over the label volume in[V] IN THE TYPE THE FILE STORES (dtype: MT_LABEL_*; int64 / uint64 files are cast
 *   to float64 on the host, as get_fdata does) -> the contiguous uint8 volume out[V].  `in` needs the alignment of its elements only
 *   and `out` none: the body starts where the input is 16-byte aligned and uses 16-byte loads, the voxels before it and after its
 *   last whole chunk (fewer than 32) are scalar accesses.  HBM-bound at itemsize bytes read and 1 byte written per voxel; no LDS.
 *   table: HOST array of MT_LABEL_SLOTS entries, built by the caller from (labels_in, labels_out) in the reference's order (the last
 *   pair that lists a label wins); table[l] is the output 0..255 of input label l, or MT_LABEL_UNLISTED.  It is passed to the
 *   kernel by value (no device table, nothing to keep alive).  Per voxel v, compared as the double it widens to:
 *     not (v > 1e-20)                         out = 0, never an error: zero, negatives, 1e-20 itself and NaN; table[0] never applies;
 *     an integer l in 1..1022 that is listed   out = table[l];
 *     anything else                            out = 0 and the voxel is UNEXPECTED: a fraction, +inf, an integer that is not listed
 *                                              or lies beyond the table.
 *   report (device uint64[2], 8-byte aligned, written by the call): report[0] = the number of unexpected voxels, report[1] = the
 *   smallest unexpected value as the bits of its double (an order-preserving key: every such value is positive), or
 *   0xffffffffffffffff when there is none.  The reference raises at the first offender of its sorted uniques, which is that value;
 *   whether unexpected voxels are an error (sanity_check) is the caller's decision.  Integer atomics only (a 64-bit add and a 64-bit
 *   min): bit-identical from run to run.  An unknown dtype, V < 1, a table entry above 255 that is not MT_LABEL_UNLISTED or a
 *   misaligned pointer is MT_EINVAL before any launch.
 * mt_label_convert_round: the voxels one full round of the grid-stride loop covers for that dtype on the current device (the launch
 *   grid is capped there); 0 for an unknown dtype. */
#define MT_LABEL_U8 0
#define MT_LABEL_I8 1
#define MT_LABEL_I16 2
#define MT_LABEL_U16 3
#define MT_LABEL_I32 4
#define MT_LABEL_U32 5
#define MT_LABEL_F32 6
#define MT_LABEL_F64 7
#define MT_LABEL_SLOTS 1023               /* input labels 0..1022, the range of mt_label_presence */
#define MT_LABEL_UNLISTED 0xffff
int mt_label_convert(const void* in, int dtype, long V, const uint16_t* table /* host */, uint8_t* out, uint64_t* report,
                     mt_stream_t stream);
long mt_label_convert_round(int dtype);
/* Training batches from cases kept on the device (training/dataloading/device_loading.py).  Additions to ABI 4.
 * mt_patch_gather: the crop and np.pad of DataLoader3D.generate_train_batch (dataset_loading.py:338-372; the box arithmetic of
 *   :259-336 stays on the host) for n <= MT_PATCH_MAX_SRC samples in ONE launch.  srcs: HOST array of n descriptors, passed to the
 *   kernel by value (no device table, no copy, nothing to keep alive but the sources themselves).  Sample j has its own source: data
 *   [C][sx, sy, sz] float32 and seg [sx, sy, sz] int16 (mt_seg_narrow), both on the device, of its own shape (a whole case, or a
 *   staged sub-box of one), and the lower corner lb of its patch in source coordinates, which may be negative.  Output voxel
 *   (j, c, d, h, w) of data_out [n, C, PD, PH, PW] reads source voxel lb + (d, h, w); outside the source it is 0 (MT_PAD_CONSTANT)
 *   or the source voxel with every coordinate clamped (MT_PAD_EDGE): np.pad's meaning for the intersection of patch and source.
 *   seg_out [n, 1, PD, PH, PW] is float32 and gets seg_fill (the loader passes -1) outside the source in either mode.  A copy: bit
 *   for bit, NaN payloads included.  data_out / seg_out need 4-byte alignment only.  A thread owns 4 consecutive w; HBM-bound at
 *   (4C + 2) bytes read and 4(C + 1) written per patch voxel.  n outside 1..16, an empty axis or a patch above INT32_MAX voxels is
 *   MT_EINVAL before any launch.
 * mt_seg_narrow: out[v] (int16, 8-byte aligned) = seg[v] for the float32 label map seg[V] (dataset_loading.py:338: the last channel
 *   of a case, small integers, -1 outside the non-zero mask).  *flag (device int32) is SET to 1 when some value is non-integral,
 *   NaN or outside int16, which is what makes the 16-bit storage lossless rather than assumed; it is never cleared by the call,
 *   so one zeroed flag can watch several calls. */
#define MT_PATCH_MAX_SRC 16
#define MT_PAD_CONSTANT 0
#define MT_PAD_EDGE 1
typedef struct {
  const float* data;   /* [C, sx, sy, sz] float32, device */
  const int16_t* seg;  /* [sx, sy, sz] labels, device */
  int32_t shape[3];    /* sx, sy, sz of THIS source */
  int32_t lb[3];       /* lower corner of the patch in source coordinates; may be negative */
} mt_patch_src_t;
int mt_patch_gather(const mt_patch_src_t* srcs /* host, n <= MT_PATCH_MAX_SRC */, int n, int C, int PD, int PH, int PW, int pad_mode,
                    float seg_fill, float* data_out, float* seg_out, mt_stream_t stream);
int mt_seg_narrow(const float* seg, long V, int16_t* out, int32_t* flag, mt_stream_t stream);
/* ---- device-side target preparation ----------------------------------------
 * Deep-supervision label pyramid: DownsampleSegForDSTransform2 / downsample_seg_for_ds_transform2 (downsampling.py:70-104,
 * order 0 = nearest through batchgenerators' resize_segmentation -> skimage.transform.resize(order 0, mode "edge") ->
 * scipy.ndimage.zoom(order 0, grid_mode=True): source index = floor((o + 0.5) * in / out), clamped) and, when
 * remove_minus_one != 0, RemoveLabelTransform(-1, 0) (data_augmentation_moreDA.py:117).  src/dst: [NC, D, H, W] float32
 * label maps (the reference's target layout [B,1,D,H,W] with NC = B). */
int mt_downsample_seg_nearest(const float* src, int NC, int Di, int Hi, int Wi, float* dst, int Do, int Ho, int Wo,
                              int remove_minus_one, mt_stream_t stream);

/* GaussianBlurTransform (data_augmentation_moreDA.py:87-88 -> scipy.ndimage.gaussian_filter per channel): ONE axis pass of the
 * separable filter, dst = correlate1d(src, w) along axis (0 D, 1 H, 2 W) with w[k] ~ exp(-k^2 / 2 sigma^2), radius int(4 sigma + 0.5),
 * 'reflect' boundaries; sigma[NC] per (sample, channel) in DEVICE memory, sigma <= 0 copies that channel.  The radius is never
 * clamped: the library cannot read a device sigma to refuse it, so a channel whose sigma needs a radius above 32 (sigma >= 8.125)
 * or is NaN gets NaN in every element of dst.  src != dst. */
int mt_gaussian_blur_axis(const float* src, float* dst, int NC, int D, int H, int W, int axis, const float* sigma, mt_stream_t stream);

/* NCDHW <-> NDHWC transposes used at the module boundary */
int mt_ncdhw_to_ndhwc(const float* in, float* out, int N, int C, long V, int ocs, mt_stream_t stream);
int mt_ndhwc_to_ncdhw(const float* in, int ics, float* out, int N, int C, long V, mt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MTSEG_H */
