/*
 * decode_png.h -- drop-in for debigulator's src/decode_png.h (src/decode_png.h:43-103),
 * served by the MI355X inflate + de-filter kernels.  Prototypes are the reference's; the
 * legacy names used by the reference's README / hellopng.c (init_PNG_decoder,
 * get_PNG_width_height, decode_PNG: src/hellopng.c:154-200) are exported as well.
 *
 * Behavioural notes:
 *   - the caller's input buffer is NOT modified (the reference packs IDAT payloads to the
 *     front of it, src/decode_png.c:1285-1291)
 *   - the reference's buffer-aliasing corruption of the last <=771 stream bytes (P2) is
 *     replayed by default so outputs are bit-identical; set the environment variable
 *     DEBIG_STRICT=1 for spec-conforming output instead
 *   - colour type 2 (RGB): the reference's output depends on a loop-nesting bug (P3) and on
 *     the PRIOR contents of out_rgba_values; it is reproduced bit for bit by default (the
 *     buffer's prior bytes are read).  DEBIG_STRICT=1 gives spec-conforming RGBA instead
 */
#ifndef DEBIG_DECODE_PNG_H
#define DEBIG_DECODE_PNG_H
#include <stdint.h>
#include <stddef.h>
#include "inflate.h"
#ifdef __cplusplus
extern "C" {
#endif

void decode_png_init(void *(*malloc_funcptr)(uint64_t __size), void (*arg_free_funcptr)(void *),
                     void *(*arg_memset_funcptr)(void *str, int c, uint64_t n),
                     void *(*arg_memcpy_func)(void *dest, const void *src, uint64_t n),
                     const uint32_t dpng_working_memory_size, const uint32_t thread_id);

void decode_png_deinit(const uint32_t thread_id);

void decode_png_get_width_height(const uint8_t *compressed_input,
                                 const uint64_t compressed_input_size, uint32_t *out_width,
                                 uint32_t *out_height, uint8_t *out_good);

void decode_png(const uint8_t *compressed_input, const uint64_t compressed_input_size,
                const uint8_t *out_rgba_values, const uint64_t rgba_values_size,
                const uint32_t thread_id, uint8_t *out_good);

/* legacy generation of the same API (thread_id 0) */
void init_PNG_decoder(void *(*malloc_funcptr)(size_t __size));
void get_PNG_width_height(const uint8_t *compressed_input, const uint64_t compressed_input_size,
                          uint32_t *out_width, uint32_t *out_height, uint32_t *out_good);
void decode_PNG(const uint8_t *compressed_input, const uint64_t compressed_input_size,
                const uint8_t *out_rgba_values, const uint64_t rgba_values_size,
                uint32_t *out_good);

/* Extension: decode n PNG files in one inflate launch + one de-filter launch.
 * outs[i] must hold out_sizes[i] == 4*w*h bytes.  Returns 0 or a HIP error code. */
int debig_decode_png_batch(const uint8_t *const *inputs, const uint64_t *input_sizes,
                           uint8_t *const *outs, const uint64_t *out_sizes, uint8_t *goods,
                           uint32_t n, const uint32_t thread_id);

/* Extension, host only (no GPU work): the container walk of decode_png (reference
 * src/decode_png.c:730-1367) on its own.  Returns 1 when decode_png would hand the file to
 * inflate() -- signature, chunk layout, IHDR/PLTE/IDAT rules, rgba_values_size == 4wh, working
 * memory large enough -- and then reports the image size, the recipient size (4wh + h + 1)
 * and the zlib payload size it would pass; 0 wherever the reference sets out_good = 0 first.
 * Chunk CRCs are NOT checked here (they are verified on the GPU by the decode calls).
 * Image dimensions whose 4wh + h + 1 does not fit 32 bits are rejected: the reference's
 * uint32 arithmetic wraps there and its de-filter loop ends in out_good = 0. */
int debig_png_probe(const uint8_t *compressed_input, const uint64_t compressed_input_size,
                    const uint64_t rgba_values_size, const uint32_t dpng_working_memory_size,
                    uint32_t *out_width, uint32_t *out_height, uint64_t *out_recipient_size,
                    uint64_t *out_zlib_size);

/* ---- beyond the reference: spec-complete PNG batch decode ------------------------------
 * decode_png() / debig_decode_png_batch above keep the reference's rules (colour types 2, 3, 6 at 8 bits, no
 * interlacing, tRNS ignored, its P2 / P3 quirks unless DEBIG_STRICT=1).  debig_png_decode_batch decodes every PNG the
 * specification allows to RGBA8 (4*w*h bytes, top-down, row-major):
 *   - signature: all 8 bytes;
 *   - chunks: IHDR first (exactly once); PLTE before the first IDAT; the IDAT chunks consecutive; IEND required, anything
 *     after it ignored; an unknown critical chunk (first letter upper case) -> E_CHUNK, unknown ancillary chunks are
 *     skipped; a chunk that runs past the end of the file -> E_CHUNK; the CRC of every chunk up to IEND is checked on
 *     the GPU -> E_CRC;
 *   - IHDR (13 bytes): (colour type, depth) in 0: 1 2 4 8 16 | 2: 8 16 | 3: 1 2 4 8 | 4: 8 16 | 6: 8 16; compression 0,
 *     filter 0, interlace 0 or 1; 1 <= w, h <= 2^31 - 1; anything else -> E_IHDR.  out_caps[i] < 4wh -> E_OUTPUT;
 *   - PLTE: required for colour type 3 and forbidden for 0 and 4 (E_CHUNK), ignored for 2 and 6; 1..256 entries,
 *     length a multiple of 3, else E_PALETTE; a palette index >= the number of entries -> E_PALETTE (found on the GPU);
 *   - tRNS (before the first IDAT): colour type 3: one alpha per palette entry, entries it does not cover get 255;
 *     0: a 16-bit grey key, 2: an RGB key, compared against the raw sample at full depth (a match: alpha 0).  A tRNS
 *     of the wrong length, before PLTE, or on colour type 4 / 6 is ignored;
 *   - zlib: CM = 8, CINFO <= 7, FCHECK, no FDICT, else E_ZLIB.  The IDAT payloads are concatenated on the device and
 *     inflated as plain RFC 1951 into exactly the scanline stream's size (per non-empty Adam7 pass
 *     h_p * (1 + ceil(w_p * channels * depth / 8))): output past it -> E_DATA_LONG, short of it -> E_DATA_SHORT, any
 *     other inflate failure -> E_INFLATE.  The Adler-32 trailer (at ceil(in_end_bits / 8)) is verified on the GPU;
 *     missing or wrong -> E_ADLER.  Bytes after the trailer are ignored;
 *     (The inflate is the library's shared one, more lenient than zlib in two places:
 *       - a block of the reserved type 3 is skipped, as by the reference, so such a stream ends in E_DATA_SHORT or E_ADLER
 *         rather than E_INFLATE;
 *       - input that runs out is an end, not an error: no symbol starts in the last byte of the span, so a stream that is
 *         cut short -- or whose last block lost its BFINAL bit, so that decoding runs on into the trailer -- ends in
 *         E_DATA_SHORT (the scanlines are incomplete) or E_ADLER (they are complete, the trailer is missing or is not
 *         where decoding stopped), not in E_INFLATE.  A cut inside a block header can still be E_INFLATE: the missing
 *         bits read as zeros and may give LEN != ~NLEN or an unusable code-length set.
 *       An over-subscribed set of code lengths (more codes of some length than the shorter ones leave room for), which the
 *       reference only asserts on, is NOT among these liberties: it is E_INFLATE, whatever kernel the batch size selects.
 *      Neither ever yields DEBIG_PNG_OK for scanlines the Adler-32 trailer does not vouch for, and neither yields a
 *      status of an earlier stage.)
 *   - pixels: a filter type > 4 -> E_FILTER; 16-bit samples reduce to their high byte; 1/2/4-bit grey scales by
 *     255/85/17; sub-byte samples are packed MSB first, every row starts on a byte boundary; grey -> (g, g, g, a).
 *     Adam7 passes (x0, y0, dx, dy) = (0,0,8,8) (4,0,8,8) (0,4,4,8) (2,0,4,4) (0,2,2,4) (1,0,2,2) (0,1,1,2).
 * Statuses are decided in this order: the chunk walk (in file order), missing PLTE / IDAT / IEND, zlib header, E_OUTPUT,
 * CRC, inflate, Adler-32, filter types, palette indices.  On error outs[i] is unspecified; other files are not affected.
 * One resource limit stands beside that promise: the device arenas of a call are sized from every file that passes the host
 * rules (its scanline size and out_bytes, as IHDR claims them), before any CRC is looked at.  A file whose IHDR claims a huge
 * image fails alone with E_OUTPUT when out_caps[i] is smaller than 4wh; when the caller offers a buffer that large and the
 * device cannot hold the arenas, the CALL returns a device error (out of memory) and no file is decoded.  Callers of untrusted
 * files bound the out_caps they are willing to offer (debig_png_info_get gives the claimed size without any allocation).
 * Routing: non-interlaced 8-bit colour type 6, and 2 without a tRNS key, go through the tuned de-filter kernels of
 * debig_decode_png_batch (spec output); everything else through the general kernel (debig_hip_png_spec_defilter_batch).
 * DEBIG_PNG_FORCE_GENERAL sends every file through the general kernel (tests, measurements).
 * Returns 0 or a device error code (then every status is unspecified). */
typedef struct debig_png_info {
    uint32_t width, height;
    uint8_t bit_depth, color_type, interlace, has_trns;
    uint32_t reserved;
} debig_png_info;

enum {
    DEBIG_PNG_OK = 0,
    DEBIG_PNG_E_SIGNATURE = 1,  /* not the 8-byte PNG signature                                 */
    DEBIG_PNG_E_CHUNK = 2,      /* chunk layout / order, unknown critical chunk, truncated file   */
    DEBIG_PNG_E_IHDR = 3,       /* IHDR length or field values                                    */
    DEBIG_PNG_E_CRC = 4,        /* a chunk's CRC-32                                               */
    DEBIG_PNG_E_ZLIB = 5,       /* zlib header                                                    */
    DEBIG_PNG_E_INFLATE = 6,    /* the DEFLATE stream is damaged                                  */
    DEBIG_PNG_E_ADLER = 7,      /* Adler-32 trailer missing or wrong                              */
    DEBIG_PNG_E_DATA_SHORT = 8, /* the stream ends before the scanlines do                        */
    DEBIG_PNG_E_DATA_LONG = 9,  /* the stream holds more than the scanlines                       */
    DEBIG_PNG_E_FILTER = 10,    /* a filter type > 4                                              */
    DEBIG_PNG_E_PALETTE = 11,   /* PLTE length, or a palette index past its entries               */
    DEBIG_PNG_E_OUTPUT = 12     /* out_caps[i] < 4wh, or the size of the requested format (or outs[i] NULL) */
};

/* Host only: signature, IHDR and the chunks up to the first IDAT -> *info (for sizing outs).  DEBIG_PNG_OK or the
 * status of the first rule broken there; info is filled as far as it was read. */
uint32_t debig_png_info_get(const uint8_t *p, uint64_t size, debig_png_info *info);

#define DEBIG_PNG_FORCE_GENERAL 1u /* test / measurements: every image through the general kernel */
int debig_png_decode_batch(const uint8_t *const *inputs, const uint64_t *input_sizes, uint8_t *const *outs,
                           const uint64_t *out_caps, uint32_t *status, debig_png_info *infos /* may be NULL */,
                           uint32_t n, uint32_t flags);

/* ---- output formats: out_format = layout | depth ---------------------------------------------------------------------
 * layout:  DEBIG_PNG_FMT_RGBA (R, G, B, A), _RGB (R, G, B), _GRAY (Y), _GRAY_ALPHA (Y, A), or _NATIVE: per image, as in
 *          the file -- colour type 0: GRAY, or GRAY_ALPHA with a tRNS key; 4: GRAY_ALPHA; 2 and 3: RGB, or RGBA with a
 *          tRNS chunk; 6: RGBA.
 * depth:   DEBIG_PNG_FMT_8 (uint8 samples), _16 (uint16, LITTLE-endian), or _NATIVE_DEPTH: 16 for 16-bit files, else 8
 *          (palette and 1/2/4-bit grey files are 8-bit).
 * out_format == 0 is RGBA8: exactly the output of debig_png_decode_batch.
 * Per pixel, in this order:
 *   1. the source samples at source precision P (16 for 16-bit files, else 8): 1/2/4-bit grey scaled to 8 bits by
 *      255/85/17, palette entries 8-bit; alpha from colour types 4 and 6, or from a tRNS that applies (palette alpha,
 *      255 for the entries it does not cover; a colour type 0/2 key: alpha 0 on a match, the maximum otherwise);
 *   2. to the output depth D: 16 -> 8 keeps the high byte, 8 -> 16 is v * 257;
 *   3. the layout, on the D-bit samples: grey from colour Y = (6968 R + 23434 G + 2366 B + 16384) >> 15; colour from
 *      grey R = G = B = Y; missing alpha is the maximum (255 or 65535); an unwanted alpha is dropped (no compositing).
 * Output: h rows of w * channels * D/8 bytes, top-down, no row padding. */
enum {
    DEBIG_PNG_FMT_RGBA = 0,
    DEBIG_PNG_FMT_RGB = 1,
    DEBIG_PNG_FMT_GRAY = 2,
    DEBIG_PNG_FMT_GRAY_ALPHA = 3,
    DEBIG_PNG_FMT_NATIVE = 4,
    DEBIG_PNG_FMT_8 = 0x00,
    DEBIG_PNG_FMT_16 = 0x10,
    DEBIG_PNG_FMT_NATIVE_DEPTH = 0x20
};
#define DEBIG_PNG_BAD_FORMAT (-1) /* debig_png_decode_batch_fmt: out_format is not layout | depth of the tables above */

/* Host only: the output of one image in out_format -- *channels (1..4) and *bytes_per_sample (1 or 2), either may be
 * NULL -- and its size in bytes, w * h * channels * bytes_per_sample in 64 bits (UINT64_MAX where that does not fit).
 * 0 for an invalid out_format (or an info without a valid colour type / depth).  Size outs[i] with debig_png_info_get and this call. */
uint64_t debig_png_out_layout(const debig_png_info *info, uint32_t out_format, uint32_t *channels,
                              uint32_t *bytes_per_sample);

/* debig_png_decode_batch to out_format: the same statuses, in the same order, and the same flags; E_OUTPUT when
 * out_caps[i] is smaller than debig_png_out_layout(&info, out_format, ...).  An out_format outside the tables returns
 * DEBIG_PNG_BAD_FORMAT and writes nothing (no status either).  debig_png_decode_batch(...) is
 * debig_png_decode_batch_fmt(..., 0).  Images whose resolved format is RGBA8 take the routing above; every other image
 * goes through the general kernel's output-format twin (debig_hip_png_spec_defilter_fmt_batch). */
int debig_png_decode_batch_fmt(const uint8_t *const *inputs, const uint64_t *input_sizes, uint8_t *const *outs,
                               const uint64_t *out_caps, uint32_t *status, debig_png_info *infos /* may be NULL */,
                               uint32_t n, uint32_t flags, uint32_t out_format);

/* ---- channel-planar output and output that stays on the device --------------------------------------------------------
 * out_layout: DEBIG_PNG_LAYOUT_HWC -- interleaved pixels, exactly debig_png_decode_batch_fmt -- or DEBIG_PNG_LAYOUT_CHW:
 * sample c of pixel (x, y) at (c * h * w + y * w + x) * bytes_per_sample; the planes follow one another without padding,
 * rows have no padding, 16-bit samples are little-endian.  The byte count is that of debig_png_out_layout.  Every image of
 * more than one channel then goes through the planar de-filter kernel (debig_hip_png_spec_defilter_planar_batch), 8-bit
 * RGB / RGBA files included; one-channel images are the same bytes in both layouts and keep their routing.  The layout is
 * an argument of its own, never a bit of out_format.  Any other out_layout (or an invalid out_format) returns
 * DEBIG_PNG_BAD_FORMAT and writes nothing. */
enum { DEBIG_PNG_LAYOUT_HWC = 0, DEBIG_PNG_LAYOUT_CHW = 1 };
#define DEBIG_PNG_BAD_ARG (-2) /* debig_png_decode_batch_dev: arena NULL, an offset not a multiple of 16, regions that overlap */

/* debig_png_decode_batch_fmt with a layout: host buffers, the same statuses, order and flags. */
int debig_png_decode_batch_layout(const uint8_t *const *inputs, const uint64_t *input_sizes, uint8_t *const *outs,
                                  const uint64_t *out_caps, uint32_t *status, debig_png_info *infos /* may be NULL */,
                                  uint32_t n, uint32_t flags, uint32_t out_format, uint32_t out_layout);

/* The same with the pixels left on the device: image i at (uint8_t *)d_out_arena + out_offs[i], at most out_caps[i] bytes
 * (E_OUTPUT is decided on the host from out_caps[i], as above).  d_out_arena is device memory of the current device.
 * Checked first, on their own, before any file is looked at and before any device work: d_out_arena NULL with n > 0, an
 * out_offs[i] that is not a multiple of 16, or two regions [out_offs[i], out_offs[i] + out_caps[i]) that overlap return
 * DEBIG_PNG_BAD_ARG and leave status unwritten.  Statuses, their order and infos are those of debig_png_decode_batch_fmt.
 * The call returns after the work has finished, so the pixels are visible to every stream; no pixel byte crosses the bus,
 * only statuses, checksum words and result structs come down.
 * What is written: the region of a file that fails on the host or before the de-filter (every status but E_FILTER and
 * E_PALETTE) is untouched; the region of a file that fails in the de-filter holds unspecified bytes inside its own
 * out_bytes = debig_png_out_layout(...); nothing outside [out_offs[i], out_offs[i] + out_bytes_i) of any file is written.
 * Not provided: animated PNGs, inputs that are already on the device, an asynchronous variant on a caller's stream. */
int debig_png_decode_batch_dev(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out_arena,
                               const uint64_t *out_offs, const uint64_t *out_caps, uint32_t *status,
                               debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags, uint32_t out_format,
                               uint32_t out_layout);

/* ---- one resized, normalised tensor for the whole batch -------------------------------------------------------------------
 * debig_png_decode_batch_tensor: bytes of n PNG files in, one dense tensor of n images of out_h x out_w pixels in device
 * memory out.  Image i occupies slot = out_h * out_w * channels * sizeof(element) bytes at (uint8_t *)d_out + i * slot, laid out
 * HWC (y, x, c) or CHW (c, y, x) without padding.  The pixels are decoded (steps 1 - 3 above, out_format concrete: no NATIVE
 * layout or depth) into an arena of the library's own on the device, then ONE launch crops, resizes and converts all images
 * (debig_hip_png_resize_batch); the call returns after the work has finished.  Nothing crosses the bus but the files, the task
 * and weight tables, statuses and checksum words.
 *
 * The arithmetic is integer up to the final conversion, so that no result depends on a summation order.  P is the source
 * precision (8 or 16: the depth of out_format), the crop is boxes[i] (w == 0 && h == 0, or boxes NULL: the whole image).
 * Weights of one axis (crop length cl, output length L, output coordinate X; Q14: >= 0, their sum exactly 16384):
 *   - interpolating (antialias off, or cl <= L): num = clamp((2X + 1) cl - L, 0, (cl - 1) 2L), i0 = num div 2L, r = num mod 2L,
 *     w1 = (r * 16384 + L) div 2L; taps {i0: 16384 - w1, i0 + 1: w1}, or the single tap {cl - 1: 16384} when i0 == cl - 1
 *     (half-pixel centres; the edges clamp inside the CROP, not the image);
 *   - antialiased (DEBIG_PNG_RESIZE_ANTIALIAS and cl > L; a triangle filter as wide as the scale): c = (2X + 1) cl; for source
 *     index j in [0, cl): n_j = 2 cl - |(2j + 1) L - c|; the taps are the j with n_j > 0; T = sum n_j,
 *     w_j = (n_j * 16384 + T div 2) div T; then 16384 - sum w_j is added to the tap with the largest n_j (the lowest such j).
 * Two passes, horizontal first:  h = sum wx_k s_k;  Hq = (h + (1 << (P - 3))) >> (P - 2)  (< 2^16);  v = sum wy_k Hq_k  (< 2^30),
 * the sample times 2^(30 - P).  The element of channel c:
 *   - DEBIG_PNG_T_UINT (uint8 for P = 8, uint16 for P = 16):  (v + (1 << (29 - P))) >> (30 - P);
 *   - DEBIG_PNG_T_F32:  (float)v, times A_c, plus B_c -- each step rounded to nearest even on its own, never a fused
 *     multiply-add -- with A_c = (float)((double)scale[c] / ((2^P - 1) * 2^(30 - P))) and B_c = bias[c]: sample01 * scale + bias;
 *   - DEBIG_PNG_T_F16 / _BF16:  that float32 converted with round to nearest even.
 * With out_w == w and out_h == h the UINT output is the cropped decode exactly, antialias on or off.  Alpha is resized like
 * any other channel: there is NO premultiplication (debig_png_decode_batch_tensor_alpha below composites or premultiplies).
 * Checked first, before any file is looked at (status unwritten): an out_format with a NATIVE layout or depth or an unknown
 * out_layout -> DEBIG_PNG_BAD_FORMAT; desc or d_out NULL with n > 0, d_out not 16-byte aligned, an unknown dtype or
 * resize_flags bit, out_w or out_h 0 or above 16384, a non-finite scale / bias with a float dtype -> DEBIG_PNG_BAD_ARG.
 * Per image: the statuses of debig_png_decode_batch_fmt in their order, and DEBIG_PNG_E_BOX, decided as soon as IHDR has been
 * read (it outranks every status found later in the file): a box with exactly one of w, h zero, a box that leaves the image
 * (64-bit sums), or antialias with cl > 64 L on either axis (that bounds the taps at 129 and keeps the corrected weight
 * positive).  E_OUTPUT: the decoded image is larger than 2^31 bytes.  A file with any non-zero status leaves its slot
 * untouched; nothing outside d_out[0 .. n * slot) is written.
 * Not provided: animated PNGs, inputs already on the device, an asynchronous variant; other filters than
 * bilinear are debig_png_decode_batch_tensor_filter's, flips, quarter turns and every other affine map are
 * debig_png_decode_batch_tensor_warp's, colour jitter (one colour matrix per file) is debig_png_decode_batch_tensor_color's,
 * autocontrast, equalize, posterize and solarize are debig_png_decode_batch_tensor_tone's, Gaussian blur and sharpness are
 * debig_png_decode_batch_tensor_blur's (all below). */
typedef struct debig_png_box { uint32_t x, y, w, h; } debig_png_box; /* w == 0 && h == 0: the whole image */
enum { DEBIG_PNG_T_UINT = 0, DEBIG_PNG_T_F32 = 1, DEBIG_PNG_T_F16 = 2, DEBIG_PNG_T_BF16 = 3 };
#define DEBIG_PNG_RESIZE_ANTIALIAS 1u
#define DEBIG_PNG_E_BOX 14 /* the crop box (rules above) */
typedef struct debig_png_tensor_desc {
    uint32_t out_w, out_h, out_format /* concrete: no NATIVE layout or depth */, out_layout /* DEBIG_PNG_LAYOUT_HWC | _CHW */;
    uint32_t dtype, resize_flags;
    float scale[4], bias[4]; /* float dtypes only */
} debig_png_tensor_desc;
int debig_png_decode_batch_tensor(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                  const debig_png_box *boxes /* may be NULL */, uint32_t *status,
                                  debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                  const debig_png_tensor_desc *desc);
/* Host only: the taps of output coordinate X by the rule above -> their number (0: cl or L zero, L > 16384, X >= L, more
 * than w_cap taps, or antialias with cl > 64 L); *first = the first tap's source index, w[0 .. count) the Q14 weights. */
uint32_t debig_png_resize_weights(uint32_t cl, uint32_t L, uint32_t antialias, uint32_t X, uint32_t *first, int16_t *w,
                                  uint32_t w_cap);

/* ---- the same tensor with the alpha channel honoured: composited over a background, or premultiplied --------------------
 * debig_png_decode_batch_tensor drops an unwanted alpha and filters straight (un-premultiplied) samples: with out_format RGB
 * a transparent file shows whatever colours its encoder left under the transparent pixels, and a shrinking resize of RGBA
 * lets those hidden colours bleed into the edges of opaque shapes.  debig_png_decode_batch_tensor_alpha takes the same
 * arguments, in the same order, and an alpha descriptor:
 *   - alpha == NULL or mode DEBIG_PNG_ALPHA_STRAIGHT: exactly debig_png_decode_batch_tensor;
 *   - DEBIG_PNG_ALPHA_OVER: desc->out_format must have layout RGB or GRAY; that is the tensor's channel set (3 or 1).  The
 *     library decodes into its arena as RGBA (for RGB) or GRAY_ALPHA (for GRAY) at the same depth by steps 1 - 3 above, and
 *     the resize launch (debig_hip_png_resize_alpha_batch) composites over background[c], one integer sample per OUTPUT
 *     channel at precision P;
 *   - DEBIG_PNG_ALPHA_PREMULTIPLIED: out_format must have layout RGBA or GRAY_ALPHA; the tensor holds premultiplied colour
 *     and plain alpha, filtered in premultiplied space.
 * The arithmetic, integer up to the one final conversion.  M = 2^P - 1, S = 30 - P, Vmax = M << S:
 *   1. premultiply every source pixel of the crop (colour s_c, alpha al):  p_c = (s_c * al + (M >> 1)) div M,  p_alpha = al;
 *   2. filter: the two passes above on p -- the same Q14 axis tables, the same Hq rounding, the same tile rules -> v_c, v_alpha;
 *   3. PREMULTIPLIED: element c is the conversion above of v_c, for every channel, alpha included;
 *   4. OVER: t = Vmax - v_alpha;  v'_c = v_c + (b_c * t + (M >> 1)) div M  (the product in 64 bits; in 32 bits, with
 *      t = q M + r:  b q + (b r + (M >> 1)) div M);  element c is the conversion above of v'_c.
 * scale[c] / bias[c] are indexed by OUTPUT channel.  p_c <= al, hence v_c <= v_alpha <= Vmax and v'_c <= Vmax: no clamp is
 * needed anywhere.  A fully opaque image gives, bit for bit, debig_png_decode_batch_tensor's RGB / GRAY result in OVER mode
 * and its RGBA / GRAY_ALPHA result in PREMULTIPLIED mode; a fully transparent one gives v'_c = b_c << S exactly.
 * Limits: premultiplying at P bits means that colour under a very low alpha keeps few bits (at alpha 1 of 255 a colour is 0
 * or 1).  That is what Pillow's "RGBa" resize does; it is harmless for OVER, whose output scales with alpha, and it is why
 * straight (un-premultiplied) output of a premultiplied resize is not offered.
 * Checked before any file is looked at, with status unwritten: every check of debig_png_decode_batch_tensor first and
 * unchanged; then DEBIG_PNG_BAD_ARG for an unknown mode, reserved != 0, a mode / layout pairing other than the ones above,
 * or, in OVER mode, a used background[c] above 2^P - 1.
 * Per image: statuses and their order, the E_BOX rule, the infos and the untouched slot of a failed file are those of
 * debig_png_decode_batch_tensor; E_OUTPUT is judged on the size of the format actually decoded (4 or 2 channels).
 * Not provided: un-premultiplied RGBA output of a premultiplied resize (it needs a division per pixel); compositing in the
 * calls that do not resize (debig_png_decode_batch_fmt, _layout, _dev); bKGD / gAMA handling (the background is the
 * caller's, the samples are composited as stored); animated PNGs. */
enum { DEBIG_PNG_ALPHA_STRAIGHT = 0, DEBIG_PNG_ALPHA_PREMULTIPLIED = 1, DEBIG_PNG_ALPHA_OVER = 2 };
typedef struct debig_png_alpha_desc {
    uint32_t mode;
    uint16_t background[4];   /* OVER: one integer sample per OUTPUT channel at precision P, 0 .. 2^P - 1 */
    uint32_t reserved;        /* 0 */
} debig_png_alpha_desc;
int debig_png_decode_batch_tensor_alpha(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                        const debig_png_box *boxes /* may be NULL */, uint32_t *status,
                                        debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                        const debig_png_tensor_desc *desc, const debig_png_alpha_desc *alpha /* may be NULL */);

/* ---- the same tensor through another filter: bicubic or nearest ---------------------------------------------------------
 * debig_png_decode_batch_tensor_filter takes the arguments of debig_png_decode_batch_tensor_alpha, in the same order, and a
 * filter descriptor.  filter == NULL or DEBIG_PNG_FILTER_BILINEAR is exactly debig_png_decode_batch_tensor_alpha: the same code
 * path, the same kernels, the same bytes.  All three alpha modes work with all three filters.  The old two calls are
 * unchanged (they still refuse resize_flags bit 1 and above).
 * Weights of one axis (crop length cl, output length L, output coordinate X; Q14, their sum exactly 16384):
 *   - DEBIG_PNG_FILTER_NEAREST: one tap, source index ((2X + 1) cl) div 2L, weight 16384.  The antialias flag is ignored (no
 *     E_BOX arises from scale).  The tiles run through the kernels of the bilinear filter; a single weight of 16384 makes both
 *     passes exact, so the UINT output is the chosen source sample ("nearest-exact" with half-pixel centres).
 *   - DEBIG_PNG_FILTER_BICUBIC: the Keys kernel with a = -1/2 (Pillow's BICUBIC; torch's bicubic with antialias=True), as wide
 *     as the scale when it shrinks with antialias; taps are clipped to the CROP and renormalised (no border replication).
 *     D = 2 cl when antialias is on and cl > L, else 2 L.  For source index j in [0, cl): m_j = |(2j + 1) L - (2X + 1) cl|; the
 *     taps are the j with m_j < 2 D (a contiguous run; a tap may carry the weight 0).  u = (m_j * 65536) div D;
 *     p = 3 u^3 - 327680 u^2 + 2^49 for u <= 65536, else p = -u^3 + 327680 u^2 - 2^35 u + 2^50 (signed 64 bits, every term
 *     below 2^55); n_j = p >> 20 (arithmetic); T = sum n_j; w_j = floor((n_j * 16384 + (T >> 1)) / T), floor toward minus
 *     infinity; then 16384 - sum w_j is added to the tap with the largest n_j (the lowest such j).  E_BOX when antialias is on
 *     and cl > 32 L on either axis (that bounds the taps at 129).  Over every cl, L in 1 .. 69 and 300 larger pairs: T > 0, at
 *     most 128 taps, weights in [-2032, 18416], sum |w_j| <= 20788 (cl = 14, L = 13); cl == L gives 16384 on the pixel itself
 *     and 0 on its neighbours, so an unscaled UINT output is the crop at P = 8 (at P = 16 see the intermediate below).
 * The signed passes (BICUBIC only; NEAREST and BILINEAR use the unsigned ones above).  M = 2^P - 1:
 *   - pass 1: h = sum wx_k s_k in signed 32 bits (|h| <= 20788 * 65535 < 2^31);
 *   - the intermediate: Hq = clamp(((h + 2^(P-2)) >> (P-1)) + 16384, 0, 65535), stored as uint16 (>> arithmetic): the sample at
 *     scale 2^15, biased, covering [-0.5, 1.5) of full scale.  The clamp is part of the definition; with sum |w| <= 20788 it is
 *     never reached.  At P = 16 it keeps 15 of the sample's 16 bits: an unscaled UINT output is min(2 * ((s + 1) >> 1), M);
 *   - pass 2: v = sum wy_k Hq_k - 2^28, signed (sum wy = 16384 exactly, so the bias leaves as one constant; |v| < 2^31);
 *   - v30 = clamp(v, 0, M << (29 - P)) << 1, and from there the ONE conversion above, unchanged: UINT, F32 (a separately
 *     rounded multiply and add), F16, BF16;
 *   - with alpha: premultiply exactly as above, filter as here; v30_alpha is clamped to [0, Vmax] first, then every v30_c to
 *     [0, v30_alpha] (with negative lobes v_c <= v_alpha no longer holds by itself); then the OVER formula or the PREMULTIPLIED
 *     output above.  A fully opaque file gives the plain bicubic result of its colour channels bit for bit, a fully
 *     transparent one the background exactly.
 * Checked before any file is looked at, with status unwritten: every check of debig_png_decode_batch_tensor_alpha first and
 * unchanged; then DEBIG_PNG_BAD_ARG for an unknown filter or reserved != 0.  Per image: statuses, their order, the untouched
 * slot of a failed file and infos are those of debig_png_decode_batch_tensor_alpha, with the E_BOX scale rule of the filter.
 * Not provided: Lanczos and other kernels, the a = -3/4 variant, border replication, animated PNGs,
 * inputs already on the device, an asynchronous variant.  (Flips and affine maps: debig_png_decode_batch_tensor_warp below;
 * colour jitter: debig_png_decode_batch_tensor_color below, for BILINEAR and NEAREST.) */
enum { DEBIG_PNG_FILTER_BILINEAR = 0, DEBIG_PNG_FILTER_BICUBIC = 1, DEBIG_PNG_FILTER_NEAREST = 2 };
typedef struct debig_png_filter_desc { uint32_t filter; uint32_t reserved; /* 0 */ } debig_png_filter_desc;
int debig_png_decode_batch_tensor_filter(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                         const debig_png_box *boxes /* may be NULL */, uint32_t *status,
                                         debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                         const debig_png_tensor_desc *desc, const debig_png_alpha_desc *alpha /* may be NULL */,
                                         const debig_png_filter_desc *filter /* may be NULL */);
/* Host only: debig_png_resize_weights for a filter (BILINEAR: that call itself) -> the number of taps; 0 as there, for an
 * unknown filter, for BICUBIC antialiased with cl > 32 L, or where T <= 0 or sum |w| > 32768 (neither occurs in the sweep
 * above). */
uint32_t debig_png_resize_weights_filter(uint32_t filter, uint32_t cl, uint32_t L, uint32_t antialias, uint32_t X,
                                         uint32_t *first, int16_t *w, uint32_t w_cap);

/* ---- label maps: palette indices and raw grey samples as one integer class-map tensor -------------------------------------
 * Segmentation masks come as palette PNGs or as 1/2/4/8/16-bit grey PNGs, and what a trainer needs from them is the palette
 * index or the grey sample itself -- which every call above destroys (a palette pixel goes through PLTE, 1/2/4-bit grey is
 * scaled by 255/85/17, 16-bit grey keeps its high byte).  debig_png_decode_batch_labels: bytes of n PNG files in, one dense
 * (n, out_h, out_w) tensor of `dtype` in device memory out; image i at (uint8_t *)d_out + i * out_h * out_w * sizeof(element),
 * no padding.  The call returns after the work has finished.
 *   - The label of a source pixel: colour type 3: the palette index (depths 1, 2, 4, 8); colour type 0: the raw sample as an
 *     unsigned number (depths 1, 2, 4, 8, 16).  Nothing is scaled; PLTE colours and any tRNS are ignored (infos[i].has_trns is
 *     still what debig_png_info_get reports); Adam7 files give the labels of their non-interlaced twins.
 *   - Geometry: the crop is boxes[i] with the box rules of debig_png_decode_batch_tensor (crop cw x chh at (bx, by)); output
 *     (X, Y) takes the source pixel (bx + ((2X + 1) cw) div 2 out_w, by + ((2Y + 1) chh) div 2 out_h) -- exactly the tap of
 *     DEBIG_PNG_FILTER_NEAREST, so a mask decoded here and an image decoded by debig_png_decode_batch_tensor_filter with the
 *     same box share one grid, whatever filter the image uses.
 *   - Value: lut[label] with a lut (256 int32 in HOST memory, read before the call returns), else the label; stored as dtype
 *     (int32 / int64 sign-extend a negative lut entry, e.g. an ignore index of -1).
 * The labels are de-filtered into the library's own device arena, one element per pixel (debig_hip_png_spec_defilter_index_batch:
 * every label file goes through it, none through the tuned kernels), then ONE launch crops, picks, remaps and widens all images
 * (debig_hip_png_label_gather_batch).
 * Checked first, before any file is looked at (status unwritten, DEBIG_PNG_BAD_ARG): desc or d_out NULL with n > 0, d_out not
 * 16-byte aligned, out_w or out_h 0 or above 16384, an unknown dtype, reserved != 0, a lut entry outside the dtype's range
 * (U8: 0 .. 255, U16: 0 .. 65535).  flags keeps its meaning (DEBIG_PNG_FORCE_GENERAL is accepted and changes nothing here).
 * Per image: the chunk walk's statuses first; as soon as IHDR has been read DEBIG_PNG_E_LABEL is decided -- colour type 2, 4
 * or 6; a 16-bit file with dtype U8; a 16-bit file with a lut -- then DEBIG_PNG_E_BOX, and both outrank anything found later in
 * the file; then the statuses of debig_png_decode_batch_fmt in their order (E_PALETTE for an index >= the PLTE entries stays,
 * found on the GPU; E_OUTPUT: the raw labels are larger than 2^31 bytes).  A file with a non-zero status leaves its slot
 * untouched; nothing outside d_out[0 .. n * slot) is written.
 * Not provided: label output to host buffers or at each file's own size, LUTs for 16-bit sources, boundary / ignore-ring
 * generation, animated PNGs, inputs already on the device, an asynchronous variant.  (Colour -> class lookup for
 * RGB-coded masks: debig_png_decode_batch_color_labels below; flips and affine maps: debig_png_decode_batch_labels_warp.) */
#define DEBIG_PNG_E_LABEL 15 /* not a label file for this call (rules above) */
enum { DEBIG_PNG_L_U8 = 0, DEBIG_PNG_L_U16 = 1, DEBIG_PNG_L_I32 = 2, DEBIG_PNG_L_I64 = 3 };
typedef struct debig_png_label_desc {
    uint32_t out_w, out_h;   /* 1 .. 16384 */
    uint32_t dtype;          /* DEBIG_PNG_L_* */
    uint32_t reserved;       /* 0 */
    const int32_t *lut;      /* host memory, 256 entries, or NULL */
} debig_png_label_desc;
int debig_png_decode_batch_labels(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                  const debig_png_box *boxes /* may be NULL */, uint32_t *status,
                                  debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                  const debig_png_label_desc *desc);

/* ---- colour-coded label maps: RGB-coded masks as one integer class-map tensor -----------------------------------------------
 * A large share of segmentation data stores the class as a COLOUR: COCO panoptic packs the segment id as R + 256 G + 65536 B,
 * Cityscapes *_color.png, Mapillary, ADE20K colour masks and most annotation-tool exports use a fixed list of RGB colours, one
 * per class, and image optimisers re-save either kind as palette or RGBA files.  debig_png_decode_batch_color_labels: bytes of
 * n PNG files in, one dense (n, out_h, out_w) tensor of `dtype` in device memory out, laid out as debig_png_decode_batch_labels
 * lays it out.  The call returns after the work has finished.
 *   - The colour of a source pixel: the three bytes debig_png_decode_batch_fmt(..., DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8) gives
 *     for it, whatever the file's colour type: palette files go through PLTE, grey is replicated (1/2/4-bit grey scaled as that
 *     call scales it), alpha and tRNS are dropped, Adam7 files give the colours of their non-interlaced twins.  The packed
 *     colour is key = R | G << 8 | B << 16.
 *   - Geometry: exactly that of debig_png_decode_batch_labels -- the box rules, the pick (bx + ((2X + 1) cw) div 2 out_w,
 *     by + ((2Y + 1) chh) div 2 out_h), d_out 16-byte aligned.
 *   - Value, mode DEBIG_PNG_CL_PACK: the element is key (COCO's rgb2id); dtype I32 or I64.
 *   - Value, mode DEBIG_PNG_CL_MAP: the element is values[k] where keys[k] == key in the image's map -- maps[0] for every image
 *     when n_maps == 1, maps[i] for image i when n_maps == n --, else `missing`; int32 / int64 sign-extend.  Maps are HOST
 *     memory, read before the call returns; the keys of one map are distinct.
 *   - unmatched (may be NULL): unmatched[i] is the exact number of OUTPUT elements of image i whose colour was not in its map
 *     (antialiased mask edges show up here); 0 in PACK mode and for a file with a non-zero status.
 * The colours are de-filtered as RGB8 into the library's own device arena (the route of debig_png_decode_batch_tensor), then ONE
 * launch picks, packs, looks up and widens all images (debig_hip_png_color_label_batch; the lookup is an open-addressing table
 * per map, made on the host once per call, staged in LDS: include/debig_hip.h).
 * Checked first, before any file is looked at (status, unmatched and tensor unwritten, DEBIG_PNG_BAD_ARG): the cases of
 * debig_png_decode_batch_labels (desc or d_out NULL with n > 0, d_out not 16-byte aligned, out_w or out_h 0 or above 16384, an
 * unknown dtype, reserved != 0); an unknown mode; PACK with dtype U8 or U16; PACK with n_maps != 0; MAP with n_maps neither 1
 * nor n, or maps NULL; a map with n > DEBIG_PNG_CMAP_MAX, or n > 0 and keys or values NULL; a key above 0xFFFFFF; two equal
 * keys in one map; a value or `missing` outside the range of dtype U8 (0 .. 255) or U16 (0 .. 65535).
 * Per image: the chunk walk's statuses first; as soon as IHDR has been read DEBIG_PNG_E_LABEL iff the file is 16-bit (its high
 * byte would pass for a colour silently), then DEBIG_PNG_E_BOX, and both outrank anything found later in the file; then the
 * statuses of debig_png_decode_batch_fmt in their order (E_PALETTE; E_OUTPUT: more than 2^31 decoded RGB8 bytes).  A file with
 * a non-zero status leaves its slot untouched; nothing outside d_out[0 .. n * slot) is written.
 * Not provided: arithmetic decodings other than PACK (e.g. ADE20K's R / 10 * 256 + G), maps above DEBIG_PNG_CMAP_MAX entries,
 * 16-bit sources, nearest-colour matching for unmatched pixels, host-buffer output, animated PNGs, inputs already on the
 * device, an asynchronous variant.  (Flips and affine maps: debig_png_decode_batch_color_labels_warp below.) */
#define DEBIG_PNG_CMAP_MAX 2048u
enum { DEBIG_PNG_CL_PACK = 0, DEBIG_PNG_CL_MAP = 1 };
typedef struct debig_png_color_map {      /* host memory, read before the call returns */
    uint32_t n;                           /* 0 .. DEBIG_PNG_CMAP_MAX */
    uint32_t reserved;                    /* (not read) */
    const uint32_t *keys;                 /* packed colours R | G << 8 | B << 16, distinct, <= 0xFFFFFF */
    const int32_t *values;
} debig_png_color_map;
typedef struct debig_png_color_label_desc {
    uint32_t out_w, out_h;                /* 1 .. 16384 */
    uint32_t dtype;                       /* DEBIG_PNG_L_* */
    uint32_t mode;                        /* DEBIG_PNG_CL_* */
    int32_t  missing;                     /* MAP: the element of a colour that is not in the image's map */
    uint32_t n_maps;                      /* MAP: 1 (one map for every image) or n (maps[i] is image i's); PACK: 0 */
    const debig_png_color_map *maps;
    uint32_t reserved;                    /* 0 */
    uint32_t reserved2;                   /* (not read) */
} debig_png_color_label_desc;
int debig_png_decode_batch_color_labels(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                        const debig_png_box *boxes /* may be NULL */, uint32_t *status,
                                        debig_png_info *infos /* may be NULL */, uint32_t *unmatched /* may be NULL */,
                                        uint32_t n, uint32_t flags, const debig_png_color_label_desc *desc);
/* Host only: the lookup table of one map as the call uploads it (include/debig_hip.h: debig_png_color_label_task has the
 * layout, the slot function and the probe rule) -> its slot count, and 2 * slots uint32 (key, value pairs) in table; 0 and
 * nothing written for a map the call refuses (map NULL, n > DEBIG_PNG_CMAP_MAX, n > 0 with a NULL array, a key above
 * 0xFFFFFF, two equal keys) or when cap_slots is too small (4096 always suffices). */
uint32_t debig_png_color_map_table(const debig_png_color_map *map, uint32_t *table, uint32_t cap_slots);

/* ---- affine warp: flips, quarter turns, rotation, scale and shear in the tensor and label decodes ---------------------------------
 * debig_png_decode_batch_tensor_warp, debig_png_decode_batch_labels_warp and debig_png_decode_batch_color_labels_warp are
 * debig_png_decode_batch_tensor, debig_png_decode_batch_labels and debig_png_decode_batch_color_labels with the resize (the
 * nearest grid) replaced by an affine map, one per file: warps[i].m is the INVERSE map M
 * (2 x 3, row major).  The continuous source position of output pixel (X, Y) is
 *     (u, v) = M . (X + 1/2, Y + 1/2, 1)
 * in pixel units of the CROP (boxes[i], or the whole image), where source pixel j covers [j, j + 1).  Singular matrices are
 * legal: the map is only ever applied in this direction.
 * The host quantises once: m_k = llround(M_k * 65536) as int64 (debig_png_warp_quantise).  A file whose matrix has a non-finite
 * entry, |M00|, |M01|, |M10| or |M11| above 32768, or |M02| or |M12| above 2^24 gets DEBIG_PNG_E_WARP; it is decided when IHDR
 * has been read, ranks behind E_LABEL and E_BOX and, like them, ahead of whatever is found later in the file.
 * All position arithmetic is int64, in Q17:
 *     U = m00 (2X + 1) + m01 (2Y + 1) + 2 m02,    V = m10 (2X + 1) + m11 (2Y + 1) + 2 m12.
 * With |m00|, |m01| <= 2^31, 2X + 1, 2Y + 1 < 2^15 and |m02| <= 2^40: |U|, |V| <= 2 * 2^31 * (2^15 - 1) + 2^41 < 2^48.
 *   - DEBIG_PNG_FILTER_NEAREST: the pick is (jx, jy) = (U >> 17, V >> 17), the shift arithmetic (floor); v30 = s << (30 - P).
 *   - DEBIG_PNG_FILTER_BILINEAR, per axis: t = U - 65536, i0 = t >> 17, f = t & 0x1FFFF, w1 = (f + 4) >> 3 (Q14, 0 .. 16384),
 *     w0 = 16384 - w1; the taps are i0 and i0 + 1.  Horizontal first, precision handling exactly as in the resize:
 *     h = w0x s(i0x) + w1x s(i0x + 1);  Hq = (h + (1 << (P - 3))) >> (P - 2);  v = w0y Hq(row i0y) + w1y Hq(row i0y + 1)  (< 2^30).
 *   - then the ONE conversion of debig_png_decode_batch_tensor, unchanged: UINT, F32 with a separately rounded multiply and
 *     add, F16, BF16; scale / bias as there.
 *   - border_mode DEBIG_PNG_BORDER_CONSTANT: a tap whose x or y lies outside [0, cl) is border[c], an integer sample at
 *     precision P per source channel (for NEAREST: an outside pick is the border); DEBIG_PNG_BORDER_CLAMP: tap indices are
 *     clamped to [0, cl - 1].  All comparisons happen in int64 before anything is narrowed.
 * Consequences: the identity matrix with out == crop gives the cropped decode exactly in UINT (f = 0: the second tap weighs 0);
 * an integer translation gives the shifted decode, with border where it leaves the crop; the flip matrices
 * ((-1, 0, cw), (0, 1, 0)) and ((1, 0, 0), (0, -1, chh)) and the quarter-turn matrices ((0, -1, cw), (1, 0, 0)),
 * ((-1, 0, cw), (0, -1, chh)), ((0, 1, 0), (-1, 0, chh)) -- numpy.rot90 with k = 1, 2, 3, into an output of chh x cw pixels
 * (w x h) for k = 1 and 3 -- give numpy.flip / numpy.rot90 of the decode exactly, for both filters (U and V are odd multiples
 * of 65536 there: f = 0 again).
 * Labels: nearest only, with the same jx, jy -- an image warped with filter NEAREST and its label map warped with the same
 * matrix pick the same source pixels.  An outside pick under CONSTANT stores border_label as it is (the ignore index: it does
 * not pass through the lut); CLAMP as above.  lut, dtypes and the E_LABEL rules are those of debig_png_decode_batch_labels.
 * Colour-coded labels: the same jx, jy again, so the colour-label call, the raw-label call and the image's NEAREST filter pick
 * the same source pixel for every output element under one matrix.  Decode, colour and key = R | G << 8 | B << 16 are those of
 * debig_png_decode_batch_color_labels.  Inside the crop, or anywhere under CLAMP, the element is the PACK or MAP value of the
 * picked pixel as in that call; an outside pick under CONSTANT stores border_label as it is (it does not pass through the map).
 * unmatched[i] is the exact number of output elements of image i that took `missing`: a border element under CONSTANT is never
 * counted, even when border_label == missing; a clamped pick goes through the map and is counted like any other; 0 in PACK
 * mode and for a file with a non-zero status.  E_LABEL is that call's (a 16-bit file).
 * All three calls decode as the calls they extend (the same arena, no crop-size cap), then ONE launch warps all images
 * (debig_hip_png_warp_batch / debig_hip_png_label_warp_batch / debig_hip_png_color_label_warp_batch: a gather, one lane per
 * output pixel).
 * Checked first, before any file is looked at (status unwritten): every check of the call that is extended, unchanged; then
 * DEBIG_PNG_BAD_ARG for warps or the warp descriptor NULL, a filter other than BILINEAR / NEAREST (BICUBIC included), an
 * unknown border_mode, alpha_mode other than DEBIG_PNG_ALPHA_STRAIGHT, reserved != 0, the antialias flag in desc->resize_flags,
 * a used border[c] above 2^P - 1 under CONSTANT, a border_label outside the dtype's range under CONSTANT (U8: 0 .. 255,
 * U16: 0 .. 65535; under CLAMP border_label is not read).  The colour-label warp leaves unmatched unwritten as well.  Per image: statuses, their order, infos and the untouched slot of a failed file are those of the call
 * that is extended, with E_WARP as above.
 * Not provided: antialiasing under a shrinking warp (shrink with the resize calls, or accept aliasing), bicubic, the OVER and
 * PREMULTIPLIED alpha modes together with a warp (alpha is warped like a colour channel, as in debig_png_decode_batch_tensor).
 * (Colour jitter under a warp: debig_png_decode_batch_tensor_warp_color below; perspective maps: the _persp calls further
 * down.) */
#define DEBIG_PNG_E_WARP 16 /* the warp matrix (rules above) */
enum { DEBIG_PNG_BORDER_CONSTANT = 0, DEBIG_PNG_BORDER_CLAMP = 1 };
typedef struct debig_png_warp { double m[6]; } debig_png_warp; /* the inverse map, row major: (m00 m01 m02) (m10 m11 m12) */
typedef struct debig_png_warp_desc {
    uint32_t filter;        /* DEBIG_PNG_FILTER_BILINEAR or DEBIG_PNG_FILTER_NEAREST */
    uint32_t border_mode;   /* DEBIG_PNG_BORDER_* */
    uint16_t border[4];     /* CONSTANT: one integer sample per source channel at precision P, 0 .. 2^P - 1 */
    uint32_t alpha_mode;    /* DEBIG_PNG_ALPHA_STRAIGHT (0): the other modes are not provided with a warp */
    uint32_t reserved;      /* 0 */
} debig_png_warp_desc;
typedef struct debig_png_label_warp_desc {
    uint32_t border_mode;   /* DEBIG_PNG_BORDER_* */
    int32_t border_label;   /* CONSTANT: the element of a pick outside the crop */
} debig_png_label_warp_desc;
/* Host only: m[k] = llround(M[k] * 65536) -> 1, or 0 (m unspecified) on the E_WARP conditions above. */
int debig_png_warp_quantise(const double M[6], int64_t m[6]);
int debig_png_decode_batch_tensor_warp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                       const debig_png_box *boxes /* may be NULL */, const debig_png_warp *warps, uint32_t *status,
                                       debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                       const debig_png_tensor_desc *desc, const debig_png_warp_desc *warp_desc);
int debig_png_decode_batch_labels_warp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                       const debig_png_box *boxes /* may be NULL */, const debig_png_warp *warps, uint32_t *status,
                                       debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                       const debig_png_label_desc *desc, const debig_png_label_warp_desc *warp_desc);
int debig_png_decode_batch_color_labels_warp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
        const debig_png_box *boxes /* may be NULL */, const debig_png_warp *warps, uint32_t *status,
        debig_png_info *infos /* may be NULL */, uint32_t *unmatched /* may be NULL */, uint32_t n, uint32_t flags,
        const debig_png_color_label_desc *desc, const debig_png_label_warp_desc *warp_desc);

/* ---- colour jitter: one 3 x 4 colour matrix per file in the tensor decodes ------------------------------------------------------
 * Brightness, contrast, saturation, hue, random grey, channel order and the negative are all one affine map of a pixel's three
 * colours.  debig_png_decode_batch_tensor_color and debig_png_decode_batch_tensor_warp_color are debig_png_decode_batch_tensor
 * (with a filter: BILINEAR, antialiased or not, or NEAREST) and debig_png_decode_batch_tensor_warp with such a map applied between
 * the filter and the ONE conversion, inside the same launch (debig_hip_png_resize_color_batch / debig_hip_png_warp_color_batch), so
 * that scale / bias still normalise the jittered sample.  colors[i].m is the matrix of file i, row major: row c is
 * (m_c0 m_c1 m_c2 | m_c3) and
 *     out_c = m_c0 R + m_c1 G + m_c2 B + m_c3,    samples in [0, 1] of full scale.
 * The host quantises once (debig_png_color_quantise; M = 2^P - 1, Vmax = M << (30 - P)):
 *     k_cj = llround(m_cj * 65536)  (int32, |k| <= 2^20),    o_c = llround(m_c3 * Vmax)  (int64; the product as float64 rounds it),
 * halves away from zero.  A file whose matrix has a non-finite entry or an entry above 16 in magnitude gets DEBIG_PNG_E_COLOR; it
 * is decided when IHDR has been read, ranks behind E_BOX and E_WARP and, like them, ahead of whatever is found later in the file.
 * The map is applied to the three colour values v_j the filter passes deliver -- the sample times 2^(30 - P), 0 .. Vmax -- in
 * 64-bit integers:
 *     acc_c = k_c0 v_0 + k_c1 v_1 + k_c2 v_2        (|acc_c| <= 3 * 2^20 * 2^30 < 2^52)
 *     v'_c  = clamp(((acc_c + 32768) >> 16) + o_c, 0, Vmax)        (the shift arithmetic: floor)
 * and v'_c takes the place of v_c in the ONE conversion of debig_png_decode_batch_tensor, unchanged: UINT, F32 with a separately
 * rounded multiply and add, F16, BF16.  The fourth channel of RGBA (alpha) is not mixed: it passes through untouched.  There is ONE
 * clamp, after the whole matrix.  torchvision's ColorJitter applies its operations one after the other and clamps to [0, 1] after
 * each; a matrix that composes them (brightness 1.5, then contrast 0.5) keeps the values that an intermediate clamp would have cut
 * off, so the two differ wherever an intermediate result leaves [0, 1].  That is on purpose: no information is lost between steps.
 * Consequences (all bit for bit, in every dtype):
 *   - the identity matrix gives the call without a matrix: ((v << 16) + 32768) >> 16 == v;
 *   - a permutation matrix gives that call with its colour channels permuted (scale / bias stay with the OUTPUT channel);
 *   - a zero matrix with an offset gives the constant clamp(o_c, 0, Vmax);
 *   - the negative (-I, offsets 1) gives v'_c = Vmax - v_c exactly: where the filter is exact (out == crop, or NEAREST) the UINT
 *     element is M - s.
 * Under a warp a CONSTANT border sample is mixed like any other sample.
 * Checked first, before any file is looked at (status unwritten): every check of the call that is extended, unchanged -- those
 * of debig_png_decode_batch_tensor, then an unknown filter or filter->reserved != 0; those of debig_png_decode_batch_tensor_warp
 * (its alpha_mode check included) --; then DEBIG_PNG_BAD_ARG for colors NULL, an out_format whose layout is not RGB or RGBA, and
 * DEBIG_PNG_FILTER_BICUBIC.  debig_png_decode_batch_tensor_color has no alpha descriptor: alpha is STRAIGHT.  Per image: statuses,
 * their order, infos and the untouched slot of a failed file are those of the call that is extended, with E_COLOR as above.
 * Not provided: bicubic, the OVER and PREMULTIPLIED alpha modes together with a matrix, grey outputs, intermediate clamps
 * between the operations a matrix composes, hue as a rotation in HSV (torchvision's; here it is a rotation about the grey axis,
 * as in DALI), contrast about the image's own mean.  (Operations that reduce over the image first -- autocontrast, equalize --
 * and the table operations posterize and solarize: debig_png_decode_batch_tensor_tone below.) */
#define DEBIG_PNG_E_COLOR 17 /* the colour matrix (rules above) */
typedef struct debig_png_color { double m[12]; } debig_png_color; /* row major: (m00 m01 m02 | m03) (m10 ..) (m20 ..) */
/* Host only: k[3 c + j] = llround(M[4 c + j] * 65536), o[c] = llround(M[4 c + 3] * Vmax) at precision bits (8 or 16) -> 1, or 0
 * (k, o unspecified) on the E_COLOR conditions above or for other bits. */
int debig_png_color_quantise(const double M[12], uint32_t bits, int32_t k[9], int64_t o[3]);
int debig_png_decode_batch_tensor_color(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                        const debig_png_box *boxes /* may be NULL */, const debig_png_color *colors, uint32_t *status,
                                        debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                        const debig_png_tensor_desc *desc, const debig_png_filter_desc *filter /* may be NULL */);
int debig_png_decode_batch_tensor_warp_color(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                             const debig_png_box *boxes /* may be NULL */, const debig_png_warp *warps,
                                             const debig_png_color *colors, uint32_t *status, debig_png_info *infos /* may be NULL */,
                                             uint32_t n, uint32_t flags, const debig_png_tensor_desc *desc,
                                             const debig_png_warp_desc *warp_desc);

/* ---- tone curves: autocontrast, equalize, posterize, solarize and caller's tables in the tensor decodes --------------------------
 * The operation lists of RandAugment, AutoAugment and TrivialAugment are the geometric and colour-matrix operations above plus
 * four per-channel look-up tables of 256 entries on the 8-bit image; two of them are computed from the image's own histogram.
 * debig_png_decode_batch_tensor_tone is the tensor call that its optional arguments select --
 *     warps == NULL, colors == NULL: debig_png_decode_batch_tensor_filter (boxes, alpha, filter as there);
 *     colors only:                   debig_png_decode_batch_tensor_color  (filter as there; alpha must be NULL);
 *     warps only:                    debig_png_decode_batch_tensor_warp   (warp_desc as there; alpha and filter must be NULL);
 *     both:                          debig_png_decode_batch_tensor_warp_color
 * -- with one tone operation per file, tones[i] = {op, param}:
 *     DEBIG_PNG_TONE_NONE          param 0          nothing: the file's slot is, bit for bit, what the extended call writes
 *     DEBIG_PNG_TONE_AUTOCONTRAST  param 0          stretch every colour channel's occupied range to 0 .. 255
 *     DEBIG_PNG_TONE_EQUALIZE      param 0          equalise every colour channel's histogram
 *     DEBIG_PNG_TONE_POSTERIZE     bits, 1 .. 8     keep the high `bits` bits
 *     DEBIG_PNG_TONE_SOLARIZE      threshold, 0 .. 256   invert the samples at or above the threshold
 *     DEBIG_PNG_TONE_TABLE         index < n_tables the caller's table `tables + 256 * param` (host memory, read before the call
 *                                                   returns), one table for every colour channel
 * Any other op or param gives the file DEBIG_PNG_E_TONE; it is decided when IHDR has been read, ranks behind E_BOX, E_WARP and
 * E_COLOR and, like them, ahead of whatever is found later in the file.
 * Where it acts: on the 8-bit result of everything the extended call does -- crop, filter or warp, colour matrix, and the
 * DEBIG_PNG_T_UINT conversion, which gives a sample s in 0 .. 255 per element.  This rounding to 8 bits between the geometric /
 * colour step and the tone step is on purpose: it is what a Pillow pipeline does and it makes the histograms well defined.  The
 * table is applied per colour channel; the last channel of RGBA / GRAY_ALPHA tensors is alpha, is not counted in any histogram
 * and passes through unchanged.  The ONE conversion of debig_png_decode_batch_tensor is then applied to
 *     v = LUT_c[s] << 22        (the sample times 2^(30 - P) at P = 8):
 * UINT gives LUT_c[s]; F32 is (float)v * A_c + B_c with a separately rounded multiply and add; F16 / BF16 as there.  A file whose
 * op is NONE does not go through the 8-bit intermediate at all.
 * The tables (debig_png_tone_table).  h_c[0 .. 255] is the count of the sample values of colour channel c over ALL out_h x out_w
 * elements of the file's image, elements that a CONSTANT warp border produced included (counts fit 32 bits: out_w, out_h <= 16384).
 *   EQUALIZE (Pillow's ImageOps.equalize, exactly): nz = the non-zero bins in order, S = sum(nz) - nz[last], step = S div 255.
 *       Fewer than 2 non-zero bins, or step == 0: the identity.  Otherwise n_0 = step div 2, n_(i+1) = n_i + h[i],
 *       lut[i] = min(n_i div step, 255)  (the min is what Pillow's point() does with entries above 255; they occur: a 20 x 20
 *       noise image has step 1 and entries up to 400).
 *   AUTOCONTRAST (cutoff 0): lo / hi = the lowest / highest non-empty bin; hi <= lo: the identity.  Otherwise
 *       lut[i] = 0 for i < lo,  clamp(((i - lo) * 255) div (hi - lo), 0, 255) for i >= lo:
 *       exact integer arithmetic, so lo -> 0 and hi -> 255 always.  Pillow's ImageOps.autocontrast evaluates
 *       int(i * (255.0 / (hi - lo)) - lo * (255.0 / (hi - lo))) in doubles, which lands one BELOW at some points where
 *       (i - lo) * 255 is an exact multiple of hi - lo (lo = 0, hi = 25, i = 25 gives 254): 12,094 of the 8,355,840 entries over all
 *       (lo, hi, i) differ, every one at such a point and by exactly 1.  That is on purpose: the brightest sample reaches 255.
 *   POSTERIZE: lut[i] = i & ~(2^(8 - bits) - 1).    SOLARIZE: lut[i] = i < threshold ? i : 255 - i.    TABLE: the caller's bytes.
 * The device builds the EQUALIZE / AUTOCONTRAST tables from a histogram it takes itself (debig_hip_png_tone_hist_batch, then
 * debig_hip_png_tone_apply_batch; integer adds, so the histogram is exact whatever the order); they equal debig_png_tone_table's.
 * Checked first, before any file is looked at (status unwritten): every check of the call that is extended, unchanged and in its
 * order (see the list above for the arguments that must then be NULL; warp_desc must be given exactly when warps is: all
 * DEBIG_PNG_BAD_ARG); then DEBIG_PNG_BAD_ARG for tones NULL, a 16-bit out_format, alpha mode PREMULTIPLIED (a tone curve on
 * premultiplied colour means nothing; OVER and STRAIGHT are fine) and tables NULL with n_tables > 0.  Per image: statuses, their
 * order, infos and the untouched slot of a failed file are those of the call that is extended, with E_TONE as above.
 * Not provided: 16-bit tensors, autocontrast's cutoff / ignore / preserve_tone, one caller's table per channel, torchvision's
 * contrast about the image's mean, tone curves in the decode calls that do not write a tensor. */
#define DEBIG_PNG_E_TONE 18 /* the tone operation (rules above) */
#define DEBIG_PNG_TONE_NONE 0u
#define DEBIG_PNG_TONE_AUTOCONTRAST 1u
#define DEBIG_PNG_TONE_EQUALIZE 2u
#define DEBIG_PNG_TONE_POSTERIZE 3u
#define DEBIG_PNG_TONE_SOLARIZE 4u
#define DEBIG_PNG_TONE_TABLE 5u
typedef struct debig_png_tone { uint32_t op; uint32_t param; } debig_png_tone;
/* Host only: the table of one channel for op / param from its histogram (ignored by POSTERIZE and SOLARIZE; may then be NULL) -> 1,
 * or 0 (lut unspecified) on the E_TONE conditions above and for NONE and TABLE, which have no table of their own. */
int debig_png_tone_table(uint32_t op, uint32_t param, const uint32_t hist[256], uint8_t lut[256]);
int debig_png_decode_batch_tensor_tone(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                       const debig_png_box *boxes /* may be NULL */, const debig_png_warp *warps /* may be NULL */,
                                       const debig_png_color *colors /* may be NULL */, const debig_png_tone *tones,
                                       const uint8_t *tables /* n_tables x 256 bytes; may be NULL when n_tables == 0 */,
                                       uint32_t n_tables, uint32_t *status, debig_png_info *infos /* may be NULL */, uint32_t n,
                                       uint32_t flags, const debig_png_tensor_desc *desc,
                                       const debig_png_alpha_desc *alpha /* may be NULL */,
                                       const debig_png_filter_desc *filter /* may be NULL */,
                                       const debig_png_warp_desc *warp_desc /* exactly when warps is given */);

/* ---- Gaussian blur and sharpness in the tensor decodes ---------------------------------------------------------------------------
 * The two neighbourhood filters of the augmentation lists: Sharpness (RandAugment, AutoAugment: Pillow's ImageEnhance.Sharpness)
 * and the Gaussian blur of SimCLR / BYOL / DINO / MoCo-v3 (torchvision's GaussianBlur; after colour jitter, before normalisation).
 * debig_png_decode_batch_tensor_blur is debig_png_decode_batch_tensor_tone -- the tensor call that warps, colors, alpha, filter
 * and warp_desc select, with its tone operations; here tones may be NULL (no file has one; tables may then be NULL too) -- with
 * one more operation per file, blurs[i] = {op, ksize, value}:
 *     DEBIG_PNG_BLUR_NONE       ksize, value ignored             nothing: the file's slot is, bit for bit, what the tone call (or,
 *                                                                with tones NULL, the extended call) writes
 *     DEBIG_PNG_BLUR_GAUSSIAN   ksize odd, 3 .. 63; value = sigma, finite, 0 < sigma <= 1000
 *     DEBIG_PNG_BLUR_SHARPNESS  value = factor, finite, |factor| <= 16; ksize ignored
 * Any other op, ksize or value gives the file DEBIG_PNG_E_BLUR; it is decided when IHDR has been read, ranks behind E_BOX, E_WARP,
 * E_COLOR and E_TONE and, like them, ahead of whatever is found later in the file.
 * Where it acts: on the 8-bit samples p that everything in front gives -- crop, filter or warp, colour matrix, the
 * DEBIG_PNG_T_UINT conversion and the file's tone table --, of the whole out_h x out_w image.  It produces v, the sample in Q22
 * (the sample times 2^22, at most 255 << 22), to which the ONE conversion of debig_png_decode_batch_tensor is applied as in the
 * tone call: UINT gives (v + 2^21) >> 22; F32 is (float)v * A_c + B_c with a separately rounded multiply and add; F16 / BF16 as
 * there.  Float outputs therefore keep the precision below one 8-bit step; UINT rounds once.
 * GAUSSIAN, on every channel, alpha included (as torchvision's GaussianBlur treats a 4-channel tensor), r = ksize div 2:
 *   weights (debig_png_blur_weights): w_j = exp(-(j / sigma)^2 / 2) for j = -r .. r in doubles, divided by their sum;
 *       q_j = floor(w_j * 16384 + 1/2); then 16384 - sum(q) is added to the centre tap q_0.  The taps are symmetric, not
 *       negative, and sum to exactly 16384;
 *   borders: mirrored without repeating the edge sample (torchvision's "reflect", scipy's "mirror"), made total by folding with
 *       period 2 (n - 1): fold(i) = m if m < n else 2 (n - 1) - m, with m = i mod 2 (n - 1) (not negative); n == 1: always 0.  A
 *       radius larger than the image is therefore defined;
 *   horizontal: h = sum_j q_j * p[y][fold(x + j)],  h16 = (h + 32) >> 6            (at most 65280: 16 bits);
 *   vertical:   v = sum_j q_j * h16[fold(y + j)][x]                               (at most 65280 << 14 = 255 << 22).
 *   v / 2^22 is within 0.05 of an 8-bit step of the mirrored separable convolution in doubles on the images tested (0.0233
 *   measured on noise, 0.0406 on blocks of 0 and 255; tests/test_png_blur_cpu.py).
 * SHARPNESS, on the colour channels only; the last channel of RGBA / GRAY_ALPHA tensors passes through (v = p << 22), as in Pillow:
 *   s = (2 * sum_9 k * p + 13) div 26 with k = (1 1 1; 1 5 1; 1 1 1) for 1 <= x <= out_w - 2 and 1 <= y <= out_h - 2, and s = p on
 *       the one-pixel border ring (everywhere when out_w < 3 or out_h < 3): Pillow's ImageFilter.SMOOTH exactly (13 is odd: no ties);
 *   K = llround(factor * 65536),  v = clamp((s << 22) + K * (p - s) * 64, 0, 255 << 22) in 64-bit integers.
 *   Factor 1 is the identity and factor 0 is SMOOTH, both exactly; the UINT result is within 1 of ImageEnhance.Sharpness, which
 *   truncates a float blend where this rule rounds.
 * Checked first, before any file is looked at (status unwritten): every check of the tone call, unchanged and in its order, except
 * that tones may be NULL; DEBIG_PNG_BAD_ARG for blurs NULL.  Like a tone operation, a blur operation goes with 8-bit out_formats
 * and alpha modes STRAIGHT and OVER.  Per image: statuses, their order, infos and the untouched slot of a failed file are those
 * of the tone call, with E_BLUR as above.
 * Not provided: 16-bit tensors, other sigmas per axis, other border rules, kernels above 63 taps, unsharp masking with a radius. */
#define DEBIG_PNG_E_BLUR 19 /* the blur operation (rules above) */
#define DEBIG_PNG_BLUR_NONE 0u
#define DEBIG_PNG_BLUR_GAUSSIAN 1u
#define DEBIG_PNG_BLUR_SHARPNESS 2u
typedef struct debig_png_blur { uint32_t op; uint32_t ksize; double value; } debig_png_blur;
/* Host only: the ksize Q14 taps of GAUSSIAN in q[0 .. ksize), zeros behind them -> 1, or 0 (q unspecified) on the E_BLUR
 * conditions above. */
int debig_png_blur_weights(uint32_t ksize, double sigma, int16_t q[63]);
int debig_png_decode_batch_tensor_blur(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                       const debig_png_box *boxes /* may be NULL */, const debig_png_warp *warps /* may be NULL */,
                                       const debig_png_color *colors /* may be NULL */, const debig_png_tone *tones /* may be NULL */,
                                       const uint8_t *tables /* n_tables x 256 bytes; may be NULL when n_tables == 0 */,
                                       uint32_t n_tables, const debig_png_blur *blurs, uint32_t *status,
                                       debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                       const debig_png_tensor_desc *desc, const debig_png_alpha_desc *alpha /* may be NULL */,
                                       const debig_png_filter_desc *filter /* may be NULL */,
                                       const debig_png_warp_desc *warp_desc /* exactly when warps is given */);

/* ---- perspective warp: keystone, homography, RandomPerspective in the tensor and both label decodes -------------------------------
 * debig_png_decode_batch_tensor_persp, debig_png_decode_batch_labels_persp and debig_png_decode_batch_color_labels_persp are the
 * affine-warp calls with the map made projective: persps[i].m is the INVERSE 3 x 3 matrix M of file i, row major.  The output
 * pixel centre p = (X + 1/2, Y + 1/2, 1) maps to
 *     (u, v) = (M0 . p / M2 . p,  M1 . p / M2 . p)
 * in pixel units of the CROP, source pixel j covering [j, j + 1): the conventions of the affine warp.
 * The host quantises once (debig_png_persp_quantise): rows 0 and 1 exactly as debig_png_warp_quantise does (Q16, the same limits);
 * row 2 as p_k = llround(M_2k * 2^30), halves away from zero.  A non-finite entry or |M_2k| > 4 fails the quantisation.
 * Per output pixel, all in int64, with cx = 2X + 1 and cy = 2Y + 1:
 *     NU = m00 cx + m01 cy + 2 m02,  NV = m10 cx + m11 cy + 2 m12    (the affine U and V: |N| < 2^48)
 *     D  = p0 cx + p1 cy + 2 p2                                        (Q31: 1.0 is 2^31)
 * D must lie in [2^21, 2^33 - 1] for EVERY pixel of the output.  D is linear in X and Y, so it is checked at the four corner
 * pixels of the out_w x out_h output (debig_png_persp_range): by the host per file, by the kernel per task.  A file that fails
 * the quantisation or the range gets DEBIG_PNG_E_WARP, at the rank and moment of the affine E_WARP: this is the case of a
 * horizon that crosses or nearly touches the output.  So no pixel ever meets a horizon, and CLAMP has no special case.
 *     U = floor(NU 2^31 / D)   in Q17, without 128-bit arithmetic:
 *         q1 = floor(NU / D)                       (floor, not truncation: NU may be negative, D > 0)
 *         r1 = NU - q1 D                           (in [0, D))
 *         U  = (q1 << 31) + ((uint64)r1 << 31) / D
 *     r1 << 31 < 2^64 because D < 2^33; |q1| <= 2^27 because D >= 2^21, so |U| < 2^59.  V likewise from NV.
 * Everything behind (U, V) is the affine warp's, word for word: the NEAREST pick (U >> 17, V >> 17), the BILINEAR taps and Q14
 * weights from U - 65536, the CONSTANT and CLAMP borders decided in int64 before anything is narrowed, the horizontal pass
 * rounded to 16 bits, the vertical pass into 30, the ONE conversion; labels, colour labels, border_label and unmatched.
 * Consequences: with row 2 = (0, 0, 1), D is 2^31 at every pixel and U, V are the affine rule's bit for bit, so such a matrix
 * gives the bytes of the _warp call of the same kind; multiplying all nine entries by 2 or by 1/2 changes no U or V (while the
 * limits hold); an image under NEAREST, its label map and its colour-coded mask pick the same source pixel under one matrix.
 * debig_png_decode_batch_tensor_persp takes the arguments of debig_png_decode_batch_tensor_blur with persps (required) in place of
 * warps and without the alpha and filter descriptors: filter, border and alpha mode are warp_desc's (required).  colors, tones,
 * tables / n_tables and blurs may each be NULL / 0; what is given selects the affine call whose argument checks (in their order),
 * statuses, infos, untouched slot of a failed file and colour / tone / blur semantics hold: _tensor_blur with blurs, else
 * _tensor_tone with tones, else _tensor_warp_color with colors, else _tensor_warp.  The two label calls take the arguments and
 * rules of debig_png_decode_batch_labels_warp and debig_png_decode_batch_color_labels_warp.  One launch warps all images
 * (debig_hip_png_persp_batch / _persp_color / _label_persp / _color_label_persp: the warp kernels with four 64-bit divisions per
 * pixel in their walk).
 * Not provided: what the affine warp does not provide, and homographies whose horizon crosses the output (E_WARP, above). */
typedef struct debig_png_persp { double m[9]; } debig_png_persp; /* the inverse map, row major */
/* Host only: m[0 .. 5] as debig_png_warp_quantise, m[6 + k] = llround(M[6 + k] * 2^30) -> 1, or 0 (m unspecified). */
int debig_png_persp_quantise(const double M[9], int64_t m[9]);
/* Host only: 1 when |m[6 + k]| <= 2^32, out_w and out_h are 1 .. 16384 and D lies in [2^21, 2^33 - 1] at the four corner pixels
 * of the out_w x out_h output, else 0. */
int debig_png_persp_range(const int64_t m[9], uint32_t out_w, uint32_t out_h);
int debig_png_decode_batch_tensor_persp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                        const debig_png_box *boxes /* may be NULL */, const debig_png_persp *persps,
                                        const debig_png_color *colors /* may be NULL */, const debig_png_tone *tones /* may be NULL */,
                                        const uint8_t *tables /* n_tables x 256 bytes; may be NULL when n_tables == 0 */,
                                        uint32_t n_tables, const debig_png_blur *blurs /* may be NULL */, uint32_t *status,
                                        debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                        const debig_png_tensor_desc *desc, const debig_png_warp_desc *warp_desc);
int debig_png_decode_batch_labels_persp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                        const debig_png_box *boxes /* may be NULL */, const debig_png_persp *persps, uint32_t *status,
                                        debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                        const debig_png_label_desc *desc, const debig_png_label_warp_desc *warp_desc);
int debig_png_decode_batch_color_labels_persp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
        const debig_png_box *boxes /* may be NULL */, const debig_png_persp *persps, uint32_t *status,
        debig_png_info *infos /* may be NULL */, uint32_t *unmatched /* may be NULL */, uint32_t n, uint32_t flags,
        const debig_png_color_label_desc *desc, const debig_png_label_warp_desc *warp_desc);

/* ---- elastic deformation: ElasticTransform, Rand2DElastic, the U-Net augmentation, in the tensor and both label decodes -----------
 * debig_png_decode_batch_tensor_elastic, debig_png_decode_batch_labels_elastic and debig_png_decode_batch_color_labels_elastic are
 * the affine-warp calls with a smooth displacement FIELD per file added in front of the map.  A field is a grid of
 * grid_h x grid_w nodes (elastic_desc: each 2 .. 33, the same for every file of the call); a node holds a displacement (dx, dy)
 * IN OUTPUT PIXELS.  Node j of an axis lies at output coordinate j W / (grid_w - 1) (j H / (grid_h - 1)): the nodes span the
 * output from edge to edge, so ONE field serves an image and its masks even when their source resolutions differ.  The field
 * composes with the affine map: the output sampling point is displaced first, then mapped into the crop -- one resampling, not
 * two.
 * The host quantises once (debig_png_elastic_quantise): d = llround(v * 65536), halves away from zero; v must be finite with
 * |v| <= 4096, so |d| <= 2^28.  A file with a node that fails gets DEBIG_PNG_E_WARP, at the rank and moment of the affine E_WARP
 * (no new status; E_LABEL > E_BOX > E_WARP > later, as before).
 * Cell and fraction per axis (debig_png_elastic_cell), shown for X with g = grid_w; Y likewise with H and grid_h:
 *     num = (2X + 1)(g - 1),  den = 2W,  k = num / den (always <= g - 2),  rem = num - k den,
 *     t   = (rem * 16384 + W) / den                                    (Q14, 0 .. 16384)
 * Weights (debig_png_elastic_weights): the Keys kernel with a = -1/2 (Catmull-Rom) from t in integers, t2 = t t, t3 = t2 t (int64):
 *     n_-1 = -t3 + 2 t2 2^14 - t 2^28          n_0 = 3 t3 - 5 t2 2^14 + 2 2^42
 *     n_1  = -3 t3 + 4 t2 2^14 + t 2^28        n_2 = t3 - t2 2^14
 *     w_j  = (n_j + 2^28) >> 29 (arithmetic) for three of the four; the fourth, the ANCHOR (w_0 when t < 8192, else w_1), is
 *     16384 - (the sum of the other three).
 * For every t: the sum is exactly 16384; t = 0 gives (0, 16384, 0, 0); w_j(t) = w_(1-j)(16384 - t); sum |w_j| <= 20480; every
 * weight lies within 1.5 units of 2^-14 of the real polynomial.
 * Displacement (debig_png_elastic_displacement): the nodes k - 1 .. k + 2 of each axis clamped into the grid (the edge nodes are
 * replicated),
 *     S = sum_i sum_j wy_i wx_j d[i][j]   (int64, |S| < 2^57; nothing is rounded in between, so the order does not matter)
 *     D = (S + 2^27) >> 28                (arithmetic; Q16, |D| < 2^29)
 * once for dx and once for dy.  Position, NU and NV being the affine U and V of m[]:
 *     U = NU + ((m00 Dx + m01 Dy + 2^14) >> 15),   V = NV + ((m10 Dx + m11 Dy + 2^14) >> 15)   (arithmetic; |sum| < 2^62)
 * Everything behind (U, V) is the affine warp's, word for word (picks, taps, borders, colour, labels, unmatched, the ONE
 * conversion).  Consequences:
 *   (a) a file without a field (nodes == NULL), or with a field of zeros, gets the bytes of the _warp call of the same kind;
 *   (b) a field whose nodes all hold the same whole number of pixels (a, b) gives the bytes of _warp with m02 + m00 a + m01 b and
 *       m12 + m10 a + m11 b (exact for matrices whose entries are multiples of 2^-16);
 *   (c) where t = 0 on both axes D is the node's value exactly: a 4 x 4 output under a 9 x 9 grid puts the centre of pixel (X, Y)
 *       on node (2Y + 1, 2X + 1);
 *   (d) an image under NEAREST, its label map and its colour-coded mask pick the same source pixel under one matrix and one field.
 * debig_png_decode_batch_tensor_elastic takes the arguments of debig_png_decode_batch_tensor_persp with warps (required, the affine
 * maps) in place of persps, followed by elastics (required, one entry per file) and elastic_desc (required).  colors, tones,
 * tables / n_tables and blurs may each be NULL / 0; what is given selects the affine call whose argument checks (in their
 * order), statuses, infos, untouched slot of a failed file and colour / tone / blur semantics hold: _tensor_blur with blurs, else
 * _tensor_tone with tones, else _tensor_warp_color with colors, else _tensor_warp.  The two label calls take the arguments and
 * rules of debig_png_decode_batch_labels_warp and debig_png_decode_batch_color_labels_warp, followed by the same two.  Behind the
 * checks of the affine call: elastics == NULL, elastic_desc == NULL, a grid dimension outside 2 .. 33 or a non-zero reserved word
 * is DEBIG_PNG_BAD_ARG.  One launch warps all images (debig_hip_png_elastic_batch / _elastic_color / _label_elastic /
 * _color_label_elastic); the quantised fields travel beside the tasks.
 * Not provided: elastic together with perspective, bicubic, the alpha modes the affine warp does not take, per-file grid sizes,
 * full-resolution or device-resident fields. */
typedef struct debig_png_elastic { const double *nodes; } debig_png_elastic; /* grid_h x grid_w x 2 doubles, row major, (dx, dy)
                                                                              * per node; NULL: no field */
typedef struct debig_png_elastic_desc { uint32_t grid_w, grid_h, reserved[2]; } debig_png_elastic_desc;
/* Host only: count values (2 per node) -> q[k] = llround(v[k] * 65536) -> 1, or 0 when one is not finite or above 4096 in
 * magnitude (q unspecified). */
int debig_png_elastic_quantise(const double *v, uint64_t count, int32_t *q);
/* Host only: the cell *k and the Q14 fraction *t of coordinate X on an axis of W pixels (X < W <= 16384) and g nodes (2 .. 33). */
void debig_png_elastic_cell(uint32_t X, uint32_t W, uint32_t g, uint32_t *k, uint32_t *t);
/* Host only: the four Q14 weights of the nodes k - 1 .. k + 2 at fraction t (0 .. 16384). */
void debig_png_elastic_weights(uint32_t t, int32_t w[4]);
/* Host only: the displacement (*Dx, *Dy), Q16, of output pixel (X, Y) of an out_w x out_h output under the quantised nodes q
 * (grid_h x grid_w x 2, as debig_png_elastic_quantise gives them) -> 1, or 0 when a size, X, Y or a node breaks its bound.  The
 * rule above restated; callers who move keypoints with the field can use it. */
int debig_png_elastic_displacement(const int32_t *q, uint32_t grid_w, uint32_t grid_h, uint32_t out_w, uint32_t out_h, uint32_t X,
                                   uint32_t Y, int64_t *Dx, int64_t *Dy);
int debig_png_decode_batch_tensor_elastic(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                          const debig_png_box *boxes /* may be NULL */, const debig_png_warp *warps,
                                          const debig_png_color *colors /* may be NULL */, const debig_png_tone *tones /* may be NULL */,
                                          const uint8_t *tables /* n_tables x 256 bytes; may be NULL when n_tables == 0 */,
                                          uint32_t n_tables, const debig_png_blur *blurs /* may be NULL */, uint32_t *status,
                                          debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                          const debig_png_tensor_desc *desc, const debig_png_warp_desc *warp_desc,
                                          const debig_png_elastic *elastics, const debig_png_elastic_desc *elastic_desc);
int debig_png_decode_batch_labels_elastic(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                          const debig_png_box *boxes /* may be NULL */, const debig_png_warp *warps, uint32_t *status,
                                          debig_png_info *infos /* may be NULL */, uint32_t n, uint32_t flags,
                                          const debig_png_label_desc *desc, const debig_png_label_warp_desc *warp_desc,
                                          const debig_png_elastic *elastics, const debig_png_elastic_desc *elastic_desc);
int debig_png_decode_batch_color_labels_elastic(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
        const debig_png_box *boxes /* may be NULL */, const debig_png_warp *warps, uint32_t *status,
        debig_png_info *infos /* may be NULL */, uint32_t *unmatched /* may be NULL */, uint32_t n, uint32_t flags,
        const debig_png_color_label_desc *desc, const debig_png_label_warp_desc *warp_desc,
        const debig_png_elastic *elastics, const debig_png_elastic_desc *elastic_desc);

/* ---- per-id pixel counts and bounding boxes of a label tensor -----------------------------------------------------------------------
 * What a detection, instance or panoptic loader reads off the mask after the crop and the warp: which ids are left, how many
 * pixels each keeps, and each id's tight box.  d_labels is a dense (n, out_h, out_w) tensor of DEBIG_PNG_L_* elements in device
 * memory -- what debig_png_decode_batch_labels, debig_png_decode_batch_color_labels and their _warp / _persp / _elastic forms
 * write, or any other tensor of that shape; how it was made does not matter.
 * THE RULE.  Image i has n_ids + 1 records, out[i * (n_ids + 1) + k]:
 *   - record k < n_ids covers the elements equal to k;
 *   - record n_ids ("other") covers every element that is negative or >= n_ids: a border label or `missing` of -1, an ignore
 *     value of 255, an int64 such as 2^32 + 3 (elements are compared whole, never truncated);
 *   - count is the number of elements covered, [x0, x1) x [y0, y1) their tight box in output pixels;
 *   - an id that does not occur has all five fields 0, and so has every record of an image whose status[i] != 0 (the files
 *     the decode calls left out; status NULL: no image is left out).
 * All fields are exact integers, and integer sums and maxima do not depend on order: the result is the same whatever the launch.
 * On the device a record is kept RAW (debig_hip.h: debig_png_label_stat), in a form whose empty state is all zeros and whose every
 * update is an add or a max; debig_png_label_stat_box converts one raw record of an out_w x out_h image.
 * n == 0: returns 0 and touches nothing.  DEBIG_PNG_BAD_ARG, with out unwritten, for d_labels or out NULL with n > 0, d_labels
 * not aligned to the element size, n_ids 0 or above DEBIG_PNG_LABEL_STATS_MAX_IDS, dtype above DEBIG_PNG_L_I64, out_w or out_h 0
 * or above 16384.  The call cuts row runs of 16384 elements, clears the raw records, launches once
 * (debig_hip_png_label_stats_batch) and copies them back; it is synchronous on the library's stream, like the decode calls, and
 * the caller makes sure that whoever wrote d_labels on another stream has finished.  Otherwise 0 or an error code of the device
 * layer.  Not thread safe against the tensor decodes of the same process (it uses their arenas). */
#define DEBIG_PNG_LABEL_STATS_MAX_IDS 1024u
typedef struct debig_png_label_box { uint32_t count, x0, y0, x1, y1; } debig_png_label_box;
/* raw: the five uint32 of one debig_png_label_stat (count, x_end, y_end, x_rev, y_rev) */
void debig_png_label_stat_box(const uint32_t raw[5], uint32_t out_w, uint32_t out_h, debig_png_label_box *box);
int debig_png_label_stats(const void *d_labels, uint32_t n, uint32_t out_w, uint32_t out_h, uint32_t dtype, uint32_t n_ids,
                          const uint32_t *status /* host, may be NULL */, debig_png_label_box *out /* host, n * (n_ids + 1) */);

/* ---- boundary bands of a label tensor: ignore rings, trimaps, edge targets ------------------------------------------------------------
 * Pascal-VOC-style void rings around every object, DeepLab trimaps, boundary targets, the U-Net border emphasis.  A ring cannot be
 * carried through a warp (a nearest-picked ring of width 1 or 2 is torn by rotation, doubled by magnification, lost under
 * shrinking), so it is made from the warped map: d_labels is a dense (n, out_h, out_w) tensor of DEBIG_PNG_L_* elements in device
 * memory, as for debig_png_label_stats -- what any of the label calls wrote, or a tensor made otherwise.
 * THE RULE.  A shape of radius r (1 .. 16) is its REACH TABLE reach[0 .. r], a half-width per row distance
 * (debig_png_label_boundary_reach):
 *   - DEBIG_PNG_BOUNDARY_SQUARE:  reach[d] = r                  (Chebyshev ball; 8-connected at r = 1)
 *   - DEBIG_PNG_BOUNDARY_DIAMOND: reach[d] = r - d              (L1 ball; 4-connected at r = 1: scikit-image's find_boundaries default)
 *   - DEBIG_PNG_BOUNDARY_DISK:    reach[d] = isqrt(r*r - d*d)   (Euclidean ball, integer square root)
 * Element (x, y) is a BOUNDARY element iff there is a dy with |dy| <= r and 0 <= y + dy < out_h and a dx with |dx| <= reach[|dy|]
 * and 0 <= x + dx < out_w such that the element at (x + dx, y + dy) differs from the element at (x, y).  Elements are compared
 * whole (3 and 2^32 + 3 differ); positions outside the image never make a boundary (the window is clipped, not padded); the rule
 * is symmetric, so both sides of an edge are marked (find_boundaries(mode="thick")); it equals "min != max over the clipped
 * footprint".
 *   - DEBIG_PNG_BOUNDARY_RING: out = boundary ? value : in, in the dtype of the input; `value` must be representable in it (it may
 *     equal an existing id);
 *   - DEBIG_PNG_BOUNDARY_EDGE: out = boundary ? 1 : 0, a dense uint8 (n, out_h, out_w).
 * The result is a pure function of the input.  The slot in d_out of an image whose status[i] != 0 is not written (status NULL: no
 * image is left out).  n == 0: returns 0 and touches nothing.  DEBIG_PNG_BAD_ARG, before any device work, for d_labels or d_out
 * NULL with n > 0 or not aligned to their element size, radius 0 or above 16, shape above DISK, mode above EDGE, dtype above
 * DEBIG_PNG_L_I64, out_w or out_h 0 or above 16384, a `value` outside the dtype under RING, and d_out's byte range overlapping
 * d_labels's (neighbouring tiles read what others write: in place is not defined).  The call cuts every image into tiles (32 x 32,
 * or larger where dtype and radius allow), launches once (debig_hip_png_label_boundary_batch) and is synchronous on the
 * library's stream, like debig_png_label_stats; the caller makes sure that whoever wrote d_labels on another stream has finished.
 * Otherwise 0 or an error code of the device layer.  Not thread safe against the tensor decodes of the same process (it uses
 * their arenas).  Not provided: a "transparent" value that never forms a boundary, inner- or outer-only bands,
 * radii above 16 (debig_png_label_distance below makes distance maps), in-place operation, host tensors. */
#define DEBIG_PNG_LABEL_BOUNDARY_MAX_RADIUS 16u
#define DEBIG_PNG_BOUNDARY_SQUARE 0u
#define DEBIG_PNG_BOUNDARY_DIAMOND 1u
#define DEBIG_PNG_BOUNDARY_DISK 2u
#define DEBIG_PNG_BOUNDARY_RING 0u
#define DEBIG_PNG_BOUNDARY_EDGE 1u
/* reach[0 .. radius] of the shape, the entries behind them 0; host only, integers only.  radius above 16 or an unknown shape:
 * seventeen zeros */
void debig_png_label_boundary_reach(uint32_t radius, uint32_t shape, uint8_t reach[17]);
int debig_png_label_boundary(const void *d_labels, void *d_out, uint32_t n, uint32_t out_w, uint32_t out_h, uint32_t dtype,
                             uint32_t radius, uint32_t shape, uint32_t mode, int64_t value, const uint32_t *status /* host, may be NULL */);

/* ---- exact Euclidean distance maps of a label tensor: border weights, signed distances, truncated targets, wide trimaps ---------------
 * What scipy.ndimage.distance_transform_edt does on the host, image by image.  Like a ring, a distance map cannot be carried
 * through a warp, so it is made from the warped map: d_labels is a dense (n, out_h, out_w) tensor of DEBIG_PNG_L_* elements in
 * device memory, as for debig_png_label_stats.  Elements are compared whole (3 and 2^32 + 3 differ, -1 and 255 differ).
 * THE RULE.  The SITES of element (x, y):
 *   - DEBIG_PNG_DISTANCE_DIFFERS:  every element of the image that differs from the element at (x, y).  On a binary mask: the
 *     distance to the other class, both halves of a signed distance map at once; on a multi-class map: the inside distance of
 *     every class at once;
 *   - DEBIG_PNG_DISTANCE_TO_VALUE: every element equal to `value` (scipy's distance_transform_edt(labels != value); the elements
 *     equal to `value` get 0).  uint8 and uint16 elements are 0 .. 255 / 0 .. 65535, int32 and int64 elements are signed; a `value`
 *     that the dtype cannot hold is not an error: no element equals it.
 * D2(x, y) = min over the sites (x', y') of (x - x')^2 + (y - y')^2, an exact integer of at most 2 * 16383^2.  Positions outside the
 * image are never sites.  NONE: the element has no site (a flat image under DIFFERS, an image without `value` under TO_VALUE).
 * cap is 0 (no cap) or 1 .. 32767: with a cap the result is min(D2, cap^2) and NONE gives cap^2; without one NONE gives the
 * format's "infinite" value.
 *   - DEBIG_PNG_DISTANCE_SQUARED: int32, the result itself; NONE without a cap is INT32_MAX;
 *   - DEBIG_PNG_DISTANCE_ROOT:    float32, the float32 NEAREST to the real square root of the result (round to nearest, the
 *     correctly rounded square root of the integer: (float)sqrt((double)d2), NOT sqrtf((float)d2), which rounds the argument first
 *     and differs above 2^24); NONE without a cap is +infinity.  A square root of an integer below 2^30 is an integer or lies at
 *     least 2^-36 away from every midpoint of two float32, so the double route cannot round twice to another float.
 * Identities: under DIFFERS, D2 <= r^2 is debig_png_label_boundary(radius r, DISK, EDGE) for r = 1 .. 16; under TO_VALUE it is the
 * square of distance_transform_edt(labels != value) wherever `value` occurs.
 * d_out is a dense (n, out_h, out_w) tensor of 4-byte elements.  The result is a pure function of the input.  The slot in d_out of
 * an image whose status[i] != 0 is not written (status NULL: no image is left out).  n == 0: returns 0 and touches nothing.
 * DEBIG_PNG_BAD_ARG, before any device work, for d_labels or d_out NULL with n > 0, d_labels not aligned to its element size, d_out
 * not aligned to 4, dtype above DEBIG_PNG_L_I64, sites above TO_VALUE, format above ROOT, cap above 32767, out_w or out_h 0 or above
 * 16384, and d_out's byte range overlapping d_labels's.  The call makes a row-distance plane of 2 bytes per element in the context's
 * arenas (debig_hip_png_label_distance_rows_batch), then the column pass (debig_hip_png_label_distance_cols_batch), both linear in
 * the image whatever it holds, and is synchronous on the library's stream, like debig_png_label_stats; the caller makes sure that
 * whoever wrote d_labels on another stream has finished.  Otherwise 0 or an error code of the device layer.  Not thread safe
 * against the tensor decodes of the same process (it uses their arenas).  Not provided: signed output, a stack of maps per class,
 * the index of the nearest site, anisotropic spacing, other metrics, in-place operation, host tensors. */
#define DEBIG_PNG_DISTANCE_DIFFERS 0u
#define DEBIG_PNG_DISTANCE_TO_VALUE 1u
#define DEBIG_PNG_DISTANCE_SQUARED 0u
#define DEBIG_PNG_DISTANCE_ROOT 1u
#define DEBIG_PNG_LABEL_DISTANCE_MAX_CAP 32767u
int debig_png_label_distance(const void *d_labels, void *d_out, uint32_t n, uint32_t out_w, uint32_t out_h, uint32_t dtype,
                             uint32_t sites, int64_t value, uint32_t cap, uint32_t format, const uint32_t *status /* host, may be NULL */);

/* ---- connected components of a label tensor: instance ids from a class map, split regions, specks, per-cell weights -------------------
 * What skimage.measure.label(x, background=..., connectivity=1|2) does on the host, and scipy.ndimage.label on a binary mask with
 * background 0.  A warp tears an object in two and a crop cuts one into pieces, so components are found in the warped map:
 * d_labels is a dense (n, out_h, out_w) tensor of DEBIG_PNG_L_* elements in device memory, as for debig_png_label_stats.
 * THE RULE.  Elements are compared whole (3 and 2^32 + 3 differ, -1 and 255 differ).  connectivity 4: edge neighbours; 8: edge and
 * corner neighbours.  Two elements of an image are NEIGHBOURS iff they are adjacent under the connectivity AND hold the same value;
 * a COMPONENT is a class of the transitive closure.  use_background 1: the elements equal to `background` belong to no component
 * (uint8 and uint16 elements are 0 .. 255 / 0 .. 65535, int32 and int64 elements are signed; a `background` that the dtype cannot
 * hold is not an error: nothing equals it); use_background 0: every element belongs to a component.  The FIRST of a component is the
 * smallest y * out_w + x over its elements.  d_out is a dense int32 (n, out_h, out_w) tensor:
 *   - DEBIG_PNG_COMPONENTS_FIRST:       every element gets the FIRST of its component, background -1: a canonical id that needs no
 *     numbering pass;
 *   - DEBIG_PNG_COMPONENTS_CONSECUTIVE: the components are numbered 1 .. K in increasing order of their FIRST, background 0:
 *     scipy.ndimage.label's numbering.
 * counts (host, may be NULL): counts[i] = K of image i, under both modes.  The result is a pure function of the input, whatever the
 * cut, the grid and the order of the tasks.  With components numbered 1 .. K, debig_png_label_stats(d_out, ..., num_ids K + 1) gives
 * every instance's pixel count and tight box.
 * The slot in d_out of an image whose status[i] != 0 is not written and its count is 0 (status NULL: no image is left out).
 * n == 0: returns 0 and touches nothing.  DEBIG_PNG_BAD_ARG, before any device work, for d_labels or d_out NULL with n > 0, d_labels
 * not aligned to its element size, d_out not aligned to 4, dtype above DEBIG_PNG_L_I64, connectivity other than 4 and 8, ids above
 * CONSECUTIVE, out_w or out_h 0 or above 16384, and d_out's byte range overlapping d_labels's.  The call makes a parent plane of 4
 * bytes per element and a count per task in the context's arenas and launches debig_hip_png_label_components_rows_batch, _merge,
 * _count, under CONSECUTIVE _number, and _finish (union-find; its work is not linear for every input: the depth of the trees depends on
 * the data and on the race between workgroups), reads the counts back and is synchronous on the library's stream, like
 * debig_png_label_stats; the caller makes sure that whoever wrote d_labels on another stream has finished.  Otherwise 0 or an error
 * code of the device layer.  Not thread safe against the tensor decodes of the same process (it uses their arenas).  Not provided:
 * tolerance-based (fuzzy) connectivity, a minimum-area filter (compose with debig_png_label_stats), 3-D labelling, in-place
 * operation, host tensors. */
#define DEBIG_PNG_COMPONENTS_FIRST 0u
#define DEBIG_PNG_COMPONENTS_CONSECUTIVE 1u
int debig_png_label_components(const void *d_labels, void *d_out, uint32_t n, uint32_t out_w, uint32_t out_h, uint32_t dtype,
                               uint32_t connectivity, uint32_t use_background, int64_t background, uint32_t ids,
                               const uint32_t *status /* host, may be NULL */, uint32_t *counts /* host, may be NULL */);

/* ---- PNG encode: dense tensors in device memory -> PNG files in host memory ---------------------------------------------------------
 * The way back from the decodes: predictions, label maps, instance ids (debig_png_label_components) or augmented images that live
 * on the GPU become PNG files without a copy of the pixels to the host.  d_images[i] is image i, a dense tensor of DEBIG_PNG_L_*
 * elements in device memory, (height, width, channels) under DEBIG_PNG_LAYOUT_HWC or (channels, height, width) under _CHW.
 * THE FILE is deterministic: the signature; IHDR with colour type 0 / 4 / 2 / 6 for 1 / 2 / 3 / 4 channels, or 3 with a palette,
 * depth 8 or 16, no interlace; PLTE (palette_entries x 3 bytes at side + palette_off) and tRNS (trns_entries bytes at side +
 * trns_off) when given; exactly ONE IDAT; IEND; no other chunk.  The IDAT payload is a zlib stream: the header 78 01, the DEFLATE
 * blocks, the Adler-32 of the filtered scanlines.  16-bit samples are big-endian in the file.
 * filter: DEBIG_PNG_FILTER_NONE .. _PAETH, that type for every row, or DEBIG_PNG_FILTER_ADAPTIVE: per row the type 0 .. 4 with the
 * smallest S = the sum of min(b, 256 - b) over the row's filtered bytes b, ties to the lowest type.  Filters are those of the PNG
 * specification with bpp = channels x depth / 8; the row above the first row and everything left of column 0 are zeros.
 * level: 0, stored blocks; 1, LZ77 + the fixed Huffman code.  The filtered stream is cut into chunks of DEBIG_PNG_ENCODE_CHUNK bytes
 * (debig_hip.h) that are compressed side by side, as pigz does: every chunk's blocks end on a byte boundary (an empty stored block
 * behind every chunk but the last), a chunk's matches may reach into the 32 KiB in front of it, and a level-1 chunk that is not
 * smaller than the same chunk stored is written stored, so a level-1 file is never longer than the level-0 file.  The bytes are a
 * pure function of the input.  NOT BUILT: dynamic Huffman blocks, lazy matching, levels above 1.  (In THIS call: level 2, one dynamic
 * Huffman block per chunk, is debig_png_encode_batch_dyn below; this call's surface and bytes are as they were.)
 * Statuses are per image; a failed image writes nothing to outs[i] and does not disturb the others; out_sizes[i] is the file's size,
 * 0 for a failed image (E_OUTPUT: the size that was needed).
 *   0                    the file was written
 *   DEBIG_PNG_E_ENCODE   the descriptor breaks a rule: a side of 0 or above 16384; channels outside 1 .. 4; more than one channel
 *                        with int32 / int64; a depth that does not fit the dtype (uint8: 8, uint16: 16, int32 / int64: 8 or 16); a
 *                        layout above _CHW; a palette of more than 256 entries, or with channels != 1 or depth != 8; more tRNS than
 *                        palette entries (without a palette: any); an image pointer that is NULL or not aligned to its element
 *   DEBIG_PNG_E_RANGE    found on the device: an element outside 0 .. 2^depth - 1 (int32 / int64), or not below palette_entries
 *   DEBIG_PNG_E_OUTPUT   out_caps[i] is below the file's size, or outs[i] is NULL.  debig_png_encode_bound always suffices.
 * DEBIG_PNG_BAD_ARG before any device work, statuses unwritten: a NULL array with n > 0 (side may be NULL when no descriptor has a
 * palette), a filter above 5, a level above 1.  n == 0: returns 0 and touches nothing.  Otherwise 0 or an error code of the device
 * layer.  The call launches debig_hip_png_encode_filter_batch and debig_hip_png_encode_deflate_batch, reads the chunks' byte counts
 * and the range flags back, lays the files out in a device arena (header chunks from the host, chunk outputs by debig_hip_gather),
 * takes the Adler-32 and the IDAT CRC-32 from debig_hip_checksum_batch and downloads every good file once; the host never loops
 * over pixel or stream bytes.  It is SYNCHRONOUS on the library's stream, like debig_png_label_stats; the caller makes sure that
 * whoever wrote the tensors on another stream has finished.  NOT THREAD SAFE against the tensor decodes of the same process (it
 * uses their arenas).  Not provided: 1 / 2 / 4-bit depths, Adam7, ancillary chunks other than tRNS, APNG, files left on the device,
 * host tensors, an asynchronous variant. */
#define DEBIG_PNG_E_ENCODE 20 /* the encode descriptor (rules above) */
#define DEBIG_PNG_E_RANGE 21  /* an element that the file's depth or palette cannot hold */
enum { DEBIG_PNG_FILTER_NONE = 0, DEBIG_PNG_FILTER_SUB = 1, DEBIG_PNG_FILTER_UP = 2, DEBIG_PNG_FILTER_AVERAGE = 3,
       DEBIG_PNG_FILTER_PAETH = 4, DEBIG_PNG_FILTER_ADAPTIVE = 5 };
typedef struct debig_png_encode_desc {
    uint32_t width, height;   /* 1 .. 16384 each                                                       */
    uint32_t channels;        /* 1 grey (or palette index), 2 grey + alpha, 3 RGB, 4 RGBA              */
    uint32_t dtype;           /* DEBIG_PNG_L_U8 / _U16 / _I32 / _I64                                   */
    uint32_t depth;           /* 8 or 16                                                               */
    uint32_t layout;          /* DEBIG_PNG_LAYOUT_HWC or _CHW, dense                                   */
    uint32_t palette_entries; /* 0, or 1 .. 256: colour type 3                                         */
    uint32_t trns_entries;    /* 0 .. palette_entries                                                  */
    uint64_t palette_off;     /* the palette, 3 bytes per entry, rel. to side                          */
    uint64_t trns_off;        /* the tRNS bytes, rel. to side                                          */
} debig_png_encode_desc;
uint64_t debig_png_encode_bound(const debig_png_encode_desc *d); /* bytes that always suffice for the file; 0 for a bad descriptor */
int debig_png_encode_batch(const void *const *d_images /* host array of device pointers */, const debig_png_encode_desc *descs,
                           const uint8_t *side /* host: palettes, tRNS */, void *const *outs /* host */, const uint64_t *out_caps,
                           uint64_t *out_sizes, uint32_t *status, uint32_t n, uint32_t filter, uint32_t level);
/* The same call with level 0, 1 or 2.  Levels 0 and 1 are debig_png_encode_batch byte for byte.  LEVEL 2: the chunks and the token
 * sequence of level 1 (the same greedy matcher), but every chunk is written as ONE DYNAMIC HUFFMAN BLOCK where that is smaller: the
 * device knows the exact sizes of the chunk stored, in the fixed code and in its own dynamic code (header included) before it
 * writes, and writes the dynamic block iff dynamic_bits < fixed_bits and its bytes with the trailer are below the stored bytes, else
 * exactly what level 1 writes.  So per chunk and per file level 2 <= level 1 <= level 0, and debig_png_encode_bound holds.  The code
 * lengths are a length-limited Huffman code by a rule that debig_hip.h states word for word (debig_hip_png_encode_dynamic_batch),
 * so the bytes are a pure function of the input here too.  The zlib header is 78 5E at level 2 and 78 01 below.  Everything else --
 * descriptors, statuses, filter, container, checksums, the three synchronisations, thread safety -- is the call above; the level-2
 * tasks run in rounds of DEBIG_PNG_ENCODE_ROUND_TASKS that share one device arena of token rows (at most 256 MiB), which changes
 * no byte.  DEBIG_PNG_BAD_ARG before any device work for a level above 2.  NOT BUILT: lazy matching and hash chains, levels above
 * 2, more than one block per chunk, optimal (package-merge) lengths. */
int debig_png_encode_batch_dyn(const void *const *d_images /* host array of device pointers */, const debig_png_encode_desc *descs,
                               const uint8_t *side /* host: palettes, tRNS */, void *const *outs /* host */, const uint64_t *out_caps,
                               uint64_t *out_sizes, uint32_t *status, uint32_t n, uint32_t filter, uint32_t level);
/* The same call with level 0, 1, 2 or 3.  Levels 0 .. 2 are debig_png_encode_batch_dyn byte for byte (the two calls above keep their
 * surface, their bytes and their refusal of level 3).  LEVEL 3: level 2's chunks, token rows, rounds, dynamic-code rule and choice
 * between the stored, the fixed and the dynamic block, behind ANOTHER MATCHER: beside the distances 1 and bpp and the table's
 * candidate it tries the byte above and its two neighbours -- the distances S, S - bpp and S + bpp with S = 1 + width x channels x
 * depth / 8, the length of a filtered row, where bpp < S and S + bpp <= 32768 --, and a match of 3 .. 15 bytes gives way to a longer
 * one that starts one byte later (one-step lazy matching).  debig_hip.h states the rule word for word
 * (debig_hip_png_encode_lz_batch), so the bytes are a pure function of the input.  Per chunk level 3 is never longer than stored,
 * and debig_png_encode_bound holds.  Level 3 is NOT guaranteed to be at most level 2: the tokens differ and neither matcher is run to
 * check the other.  It is made for label maps, instance ids, boundary rings and other flat tensors, above all under filter none; on
 * photographs it changes next to nothing.  The zlib header is 78 9C at level 3.  DEBIG_PNG_BAD_ARG before any device work for a
 * level above 3.  NOT BUILT: hash chains, a second or wider table, candidates beyond S +- bpp, levels above 3, more than one block
 * per chunk, optimal parsing, optimal (package-merge) lengths. */
int debig_png_encode_batch_lz(const void *const *d_images /* host array of device pointers */, const debig_png_encode_desc *descs,
                              const uint8_t *side /* host: palettes, tRNS */, void *const *outs /* host */, const uint64_t *out_caps,
                              uint64_t *out_sizes, uint32_t *status, uint32_t n, uint32_t filter, uint32_t level);

/* ---- animated PNG (APNG: acTL / fcTL / fdAT, PNG specification Third Edition) -----------------------------------------
 * A file without acTL is a still image of one frame (its fcTL / fdAT chunks are skipped as unknown ancillary chunks); its
 * output is that of debig_png_decode_batch byte for byte.  A file whose acTL is honoured fails with E_ANIM when
 *   - acTL comes after the first IDAT, comes more than once, is not 8 bytes long or has num_frames == 0;
 *   - an fcTL is not 26 bytes long, has a width or height of 0, x_off + width > W or y_off + height > H (in 64 bits),
 *     dispose_op > 2 or blend_op > 1;
 *   - more than one fcTL comes before the first IDAT, or an fcTL before it is not the whole canvas at (0, 0);
 *   - an fdAT comes before the first IDAT, is shorter than 4 bytes, or has no fcTL after the IDAT in front of it;
 *   - a frame after the IDAT has no fdAT;
 *   - the sequence numbers of fcTL and fdAT, in file order, are not 0, 1, 2, ...;
 *   - the number of fcTL differs from acTL's num_frames.
 * Every rule of debig_png_decode_batch still applies; the zlib header, inflate, data length and Adler-32 rules apply to
 * each FRAME's stream: frame 0's is the IDAT concatenation when the IDAT image is frame 0 (an fcTL before the first
 * IDAT), every other frame's the payloads of its fdAT chunks without their 4-byte sequence numbers, in file order.  A
 * frame is decoded at its own width x height with the file's colour type, depth, palette, tRNS and interlace, to RGBA8 by
 * the rules of debig_png_decode_batch.  An IDAT image that is not frame 0 is not decoded (its chunks' CRCs are checked).
 * Statuses: the order of debig_png_decode_batch with E_ANIM directly after the chunk walk; E_OUTPUT when
 * out_caps[i] < num_frames * w * h * 4; within one step the first failing frame decides (a filter error in any frame
 * outranks a palette error in any frame).
 * Compositing (APNG specification): the canvas starts as (0, 0, 0, 0); for frame k on its region R_k
 *   1. dispose_op PREVIOUS: save the canvas on R_k (on frame 0 PREVIOUS counts as BACKGROUND);
 *   2. blend_op SOURCE replaces R_k; OVER with source alpha sa: 255 takes the source, 0 keeps the canvas, otherwise
 *      u = sa * 255, v = (255 - sa) * da, al = u + v, c = (sc * u + dc * v) / al per colour channel, a = al / 255
 *      (unsigned integers, truncating division);
 *   3. output frame k is the whole canvas;
 *   4. dispose of R_k: NONE keeps it, BACKGROUND sets it to (0, 0, 0, 0), PREVIOUS restores what step 1 saved.
 * Not provided: other output formats for animations, uncomposited frames, the default image when it is not a frame. */
typedef struct debig_apng_frame {
    uint32_t width, height, x_off, y_off;   /* fcTL region on the canvas                                             */
    uint16_t delay_num, delay_den;          /* as stored (den 0 means 1/100 s by the APNG specification)              */
    uint8_t dispose_op, blend_op;           /* as stored: 0 NONE / 1 BACKGROUND / 2 PREVIOUS; 0 SOURCE / 1 OVER       */
    uint16_t reserved;
} debig_apng_frame;

typedef struct debig_apng_info {
    debig_png_info png;        /* the canvas = IHDR, as debig_png_info_get fills it          */
    uint32_t num_frames;       /* frames of the animation; 1 for a still PNG                 */
    uint32_t num_plays;        /* acTL; 0 = forever (still PNG: 0)                            */
    uint32_t default_is_frame; /* 1 when the IDAT image is frame 0 (or the file is still)     */
    uint32_t reserved;
} debig_apng_info;

#define DEBIG_PNG_E_ANIM 13 /* acTL / fcTL / fdAT rules (list above) */

/* Host only: the whole chunk walk (every fcTL), no CRCs.  DEBIG_PNG_OK or the first status of the walk, then E_ANIM;
 * info is filled as far as it was read (num_frames: acTL's, 1 for a still file).  frames may be NULL, else it receives
 * up to max_frames fcTL regions, in file order (a still file: one frame, the whole canvas, NONE / SOURCE). */
uint32_t debig_apng_info_get(const uint8_t *p, uint64_t size, debig_apng_info *info, debig_apng_frame *frames,
                             uint32_t max_frames);

/* outs[i]: num_frames * w * h * 4 bytes; frame k (the canvas after frame k is rendered, before its dispose_op) at
 * k * w * h * 4, RGBA8, rows top-down without padding.  flags: DEBIG_PNG_FORCE_GENERAL as for debig_png_decode_batch
 * (the frames take that call's de-filter routing).  Returns 0 or a device error code (then every status is unspecified). */
int debig_apng_decode_batch(const uint8_t *const *inputs, const uint64_t *input_sizes, uint8_t *const *outs,
                            const uint64_t *out_caps, uint32_t *status, debig_apng_info *infos /* may be NULL */,
                            uint32_t n, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif
