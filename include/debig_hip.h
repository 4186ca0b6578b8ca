/*
 * debig_hip.h -- C-ABI of libdebigulator_hip.so: the MI355X (gfx950) batched
 * DEFLATE inflate / PNG de-filter path behind debigulator's header API.
 *
 * Everything here is plain C: pointers, sizes, POD structs.  No HIP or torch
 * types appear in a signature; `hip_stream` is an opaque hipStream_t passed as
 * void* (NULL = the default stream).
 *
 * What each entry point replaces in the reference (ArtOfBBQ/debigulator):
 *   debig_hip_inflate_batch      N x inflate()           src/inflate.h:51-60, src/inflate.c:786-1965
 *   debig_hip_inflate_batch_ex   the same, with the number of wavefronts per stream chosen
 *                                by the caller (few large streams vs thousands of small ones)
 *   debig_hip_png_defilter_batch the de-filter + palette loops of decode_png()
 *                                                         src/decode_png.c:1381-1564
 *   debig_hip_png_decode_fused_batch  inflate + de-filter of decode_png() in one kernel
 *                                                         src/decode_png.c:800-820 -> :1381-1564
 *   debig_hip_checksum_batch     update_crc() over PNG chunks, src/decode_png.c:313-333 (and the
 *                                gzip CRC-32 / zlib Adler-32 trailers the reference never checks)
 *   debig_hip_gather             the IDAT concatenation decode_png does in the caller's buffer,
 *                                src/decode_png.c:1285-1291, as a device-to-device copy list
 * The single-call drop-in API (inflate / decode_png / decode_gz with the
 * reference's own prototypes) is in inflate.h, decode_png.h, decode_gz.h next to
 * this file and is implemented on top of these batch calls; decode_gz.h also has
 * debig_gunzip_batch, an RFC 1952-complete gunzip that goes beyond the reference.
 */
#ifndef DEBIG_HIP_H
#define DEBIG_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* One raw DEFLATE stream (what one reference inflate() call receives).  Offsets
 * are relative to the input / output arenas given to the batch call. */
typedef struct debig_stream {
    uint64_t in_off;  /* first byte of the compressed stream (any alignment)          */
    uint64_t in_len;  /* compressed_input_size (reference inflate.h:57)               */
    uint64_t out_off; /* start of the recipient (any alignment)                       */
    uint64_t out_cap; /* recipient_size (reference inflate.h:52); never written past  */
    /* decode_png() buffer-aliasing replay (reference quirk):
     * stream byte index aliased by the first scratch-table byte, and the
     * recipient size `est`.  p2_on = 0 for plain inflate()/decode_gz().          */
    int64_t p2_s0;
    uint64_t p2_est;
    uint32_t p2_on;
    uint32_t flags;   /* DEBIG_STREAM_* (0 = exactly the reference's inflate())         */
} debig_stream;

/* debig_stream.flags.  NO_REF_GATES: skip the reference's argument gates
 * (recipient_size < compressed_input_size, compressed_input_size < 5; quirk Q1) -- for
 * callers outside the reference's API whose input span is not "one stream", e.g. a gzip
 * member followed by further members (debig_gunzip_batch).  Such a span is plain RFC 1951 to its
 * caller, so one more of the reference's liberties ends with the gates: an over-subscribed set of
 * code lengths (Kraft sum above 1; the reference only asserts) fails the stream with
 * DEBIG_E_BAD_CODE_LENGTHS, in every kernel alike -- left alone, each kernel would resolve the
 * overlapping codes by its own table layout and the result would depend on the batch size. */
#define DEBIG_STREAM_NO_REF_GATES 1u
/* A HINT for the host layers' choice of path, ignored by the kernels: the stream holds filtered image rows (a PNG IDAT
 * payload).  Such data is short matches a few bytes back, chained a dozen deep: a wavefront resolves it at the latency
 * of its LDS, and what helps is more wavefronts per stream -- chunk tasks (DEBIG_WAVES_CHUNKED) -- already from
 * 256 KiB of input per stream (one sample file of the reference, 1 MB of IDAT: 28.7 ms on a workgroup of eight
 * wavefronts, 4.9 ms in chunk tasks; text of the same size is faster on the workgroup).  decode_png sets it. */
#define DEBIG_STREAM_IMAGE_ROWS 2u
/* Test hook (fault injection, never set by the host layer): the multi-wavefront match resolve
 * gives up at its first idle poll instead of after DEBIG_RESOLVE_IDLE_BOUND of them, so the
 * DEBIG_E_INTERNAL path can be exercised on ordinary data. */
#define DEBIG_STREAM_FAULT_INJECT_IDLE 0x80000000u

/* status codes in debig_result.status (0 = success) */
enum {
    DEBIG_OK = 0,
    DEBIG_E_GATE_RECIPIENT_SMALL = 1, /* recipient_size < compressed_input_size (inflate.c:826) */
    DEBIG_E_GATE_INPUT_SHORT = 2,     /* compressed_input_size < 5 (inflate.c:836)              */
    DEBIG_E_STORED_NLEN = 3,          /* LEN != ~NLEN (inflate.c:949)                           */
    DEBIG_E_BAD_CODE_LENGTHS = 4,     /* code length >= table size (inflate.c:599)             */
    DEBIG_E_NO_CODE = 5,              /* bit pattern matches no code (inflate.c:465-473)        */
    DEBIG_E_DIST_SYMBOL = 6,          /* distance symbol > 29 (inflate.c:1809)                  */
    DEBIG_E_DIST_TOO_FAR = 7,         /* distance beyond start of output (inflate.c:1843)       */
    DEBIG_E_OUTPUT_FULL = 8,          /* output would exceed recipient_size (ref: overflow/assert) */
    DEBIG_E_LITLEN_286_287 = 9,       /* symbols 286/287 (ref: reads past its table)            */
    DEBIG_E_INTERNAL = 10,            /* a kernel-internal guard tripped (bounded wait exhausted); never
                                         expected -- the stream is reported failed, not silently wrong */
    DEBIG_E_RETRY = 11                /* a throughput route (DEBIG_WAVES_SPLIT, _SPLIT_QUEUED, _STRAND, _STRAND_PIPE,
                                         _CHUNKED) handed the stream back.  Visible only under DEBIG_NO_HANDBACK (below):
                                         otherwise the workgroup-per-stream kernel launched behind the route in the same
                                         call has replaced it with the stream's own status */
};

typedef struct debig_result {
    uint64_t final_size; /* *final_recipient_size                                     */
    uint32_t good;       /* *out_good                                                 */
    uint32_t status;     /* DEBIG_E_* reason when good == 0                           */
    uint32_t final_set;  /* 0 when the reference leaves *final_recipient_size untouched */
    uint32_t n_blocks;
    uint32_t n_windows;  /* decode windows processed (perf counters, not API)          */
    uint32_t n_rounds;   /* speculative rounds summed over windows                     */
    /* shader-clock cycles per phase, only filled by -DDEBIG_PROFILE builds (else 0):
     * 0 stage input, 1 pass-1 scan rounds, 2 pass-2 decode, 3 LZ77 resolve, 4 flush,
     * 5 headers + tables, 6 whole stream, 7 far-match copy */
    uint32_t prof[8];
    /* bit position (relative to the stream's first byte) where decoding stopped: just past the
     * end-of-block code of the final block on success.  ceil(in_end_bits / 8) is where a
     * container's trailer starts (gzip CRC-32/ISIZE, zlib Adler-32). */
    uint64_t in_end_bits;
} debig_result;

/* Inflate n independent raw DEFLATE streams.  All pointers are DEVICE pointers
 * (streams/results included); the call is asynchronous on hip_stream.
 * Returns 0 or a hipError_t value. */
int debig_hip_inflate_batch(const void *d_in, void *d_out, const debig_stream *d_streams,
                            debig_result *d_results, uint32_t n, void *hip_stream);

/* Same, choosing how many 64-lane wavefronts cooperate on ONE stream:
 *   1          one wavefront per stream (best for many thousands of streams)
 *   2, 4, 8    one stream per workgroup of that many wavefronts (best for a few large
 *              streams, e.g. big PNG images; 8 uses half-size input segments)
 *   DEBIG_WAVES_LARGE4_SMALL1 / _SMALL2
 *              by stream: large ones (>= 256 KiB of input or >= 1 MiB of recipient) 4-wide,
 *              the others 1- or 2-wide, as two launches that run side by side (an internal
 *              HIP stream; hip_stream continues only after both)
 *   0          the library picks from n: n <= 256: 8; n <= 512: 4; n <= 768: 2; n <= 2048: DEBIG_WAVES_STRAND_PIPE;
 *              n <= 3072: DEBIG_WAVES_STRAND; else DEBIG_WAVES_SPLIT (never a mixed mode: stream sizes are in
 *              device memory; the host batch calls, which see the sizes, also take the pipeline for 257..768
 *              streams of 128 KiB of input or more on average).
 *              debig_hip_inflate_batch does this.
 *              The environment variable DEBIG_WAVES_PER_STREAM (1, 2, 4, 0x41, 0x42)
 *              replaces this choice, for measurements.
 * Results are identical for every choice.  Any other value: hipErrorInvalidValue. */
#define DEBIG_LARGE_IN_BYTES (256u << 10)  /* a stream is "large" from this much input ...   */
#define DEBIG_LARGE_OUT_BYTES (1u << 20)   /* ... or this much recipient (out_cap)            */
#define DEBIG_WAVES_AUTO 0u
#define DEBIG_WAVES_LARGE4_SMALL1 0x41u
#define DEBIG_WAVES_LARGE4_SMALL2 0x42u
/*   DEBIG_WAVES_SPLIT
 *              the throughput path for thousands of streams (what 0 picks for n > 1024): two
 *              kernels, one wavefront per stream each -- a scan kernel (block headers, tables,
 *              speculative Huffman scan; its decoded symbols go to a token workspace in HBM) and
 *              an LZ77 kernel (replays the tokens, resolves matches, writes the output) -- both
 *              at 3 wavefronts per SIMD instead of 2.  Needs device workspace
 *              (debig_hip_inflate_batch_ws; debig_hip_inflate_batch / _ex use a cached internal
 *              one of DEBIG_WORKSPACE_MB MiB, default 1024); a stream that does not fit its share
 *              is decoded by the one-kernel path in the same call.
 *              ORDER: one workgroup per stream is dealt to the shader engines by index, whatever it costs,
 *              so since round 4 the plan step also fixes the DISPATCH order: streams that look expensive
 *              (recipient larger than input + 64 bytes) first, stored / incompressible ones behind them, each
 *              class in the caller's order.  Stored and Huffman streams alternating in the descriptors
 *              (1.59 ms before, 1.8 x the sorted batch) now take what the sorted batch takes (0.91 vs 0.89 ms:
 *              bench.py reports both, roofline and roofline_interleaved).  What is left to the caller: batches
 *              whose expensive streams differ a lot among themselves (thumbnails beside full images): group
 *              them by size, or use DEBIG_WAVES_SPLIT_QUEUED. */
#define DEBIG_WAVES_SPLIT 0x10u
/*   DEBIG_WAVES_SPLIT_QUEUED
 *              DEBIG_WAVES_SPLIT for a batch whose ORDER mixes cheap and expensive streams (stored and
 *              Huffman streams alternating, thumbnails beside full images): workgroups that stay on
 *              the device and take streams from a queue instead of one workgroup per stream.  The
 *              hardware deals workgroups to its shader engines by index, whatever they cost, so with
 *              DEBIG_WAVES_SPLIT an alternating order can leave half the chip idle (4096 Huffman
 *              streams alternating with 4096 tiny ones: 1.67 ms, queued 0.98 ms, sorted by kind 0.89 ms).
 *              Never picked by 0: a batch sorted or grouped by kind / size is 2-4 % faster with
 *              DEBIG_WAVES_SPLIT.  DEBIG_SPLIT_WORKGROUPS overrides the number of resident workgroups. */
#define DEBIG_WAVES_SPLIT_QUEUED 0x11u
/*   DEBIG_WAVES_STRAND
 *              DEBIG_WAVES_SPLIT with the long-segment scan (csrc/inflate_strand_kernel.inc): a lane decodes a
 *              contiguous STRAND of a Huffman block as long as the block allows (a 64 KiB fixed-Huffman
 *              stream: one window of 64 strands) from a per-lane input ring in LDS, keeps its tokens in one
 *              pass, and only the lanes whose guessed start was wrong are decoded again, up to the point
 *              where they rejoin their first decode.  Same workspace, same results. */
#define DEBIG_WAVES_STRAND 0x12u
/*   DEBIG_WAVES_STRAND_PIPE
 *              DEBIG_WAVES_STRAND as a pipeline inside a workgroup of TWO wavefronts: one scans the stream, the other
 *              replays what the first has finished, record by record (a window, a stored block).  For batches that
 *              leave most SIMDs one or two wavefronts (a few hundred to about two thousand streams): a stream then
 *              takes max(scan, LZ77) instead of their sum.  Same workspace, same results. */
#define DEBIG_WAVES_STRAND_PIPE 0x13u
#define DEBIG_STRAND_MIN_STREAMS 768u  /* what 0 picks: up to here 2 wavefronts per stream ...            */
#define DEBIG_STRAND_MAX_STREAMS 3072u /* ... DEBIG_WAVES_STRAND up to here, DEBIG_WAVES_SPLIT beyond      */
#define DEBIG_STRAND_PIPE_MAX_STREAMS 2048u /* ... and up to here as a two-wavefront pipeline (DEBIG_WAVES_STRAND_PIPE) */
#define DEBIG_STRAND_PIPE_MEAN_IN_BYTES (128u << 10) /* host batch calls: 257..768 streams this long on average also take it */
/*   DEBIG_WAVES_CHUNKED
 *              a FEW LARGE streams (hundreds of big PNG images): every stream is cut at DEFLATE
 *              block boundaries into chunk tasks of 32..256 KiB of input, found by looking for
 *              dynamic block headers, and the tasks go through the scan / LZ77 kernels side by
 *              side; a task does not know the 32 KiB of output in front of it, so its matches
 *              are replayed against two synthetic histories and translated once the true window
 *              is known (csrc/inflate_chunk_kernel.inc).  Needs workspace:
 *              debig_hip_inflate_chunked_workspace_bytes(); callers with more data than
 *              workspace pass the batch in groups.  Streams the path cannot take (no dynamic
 *              blocks, a block longer than the workspace share, a failing stream, any doubt)
 *              are decoded by the one-kernel path in the same call.  Never picked by 0. */
#define DEBIG_WAVES_CHUNKED 0x20u
/* DEBIG_NO_HANDBACK (environment variable, read at every call; tests and measurements): set to anything but the empty
 * string or "0", the five routes above that hand streams back -- DEBIG_WAVES_SPLIT, _SPLIT_QUEUED, _STRAND,
 * _STRAND_PIPE and _CHUNKED, in debig_hip_inflate_batch / _ex / _ws and debig_hip_inflate_planned_ws / _ex -- do NOT
 * launch the workgroup-per-stream kernel behind themselves.  A stream the route handed back then keeps what the route
 * wrote: good = 0, status = DEBIG_E_RETRY, final_set = 0 (DEBIG_WAVES_STRAND_PIPE, whose LZ77 wavefront replays behind the
 * scan and has come some way when the scan gives up: final_set and final_size as that wavefront left them, they mean
 * nothing); its output bytes are unspecified.  Every other stream is the
 * route's own work, which is what the switch is for: without it nothing in the results says which kernel produced the
 * bytes.  Where a call would send the WHOLE batch to the workgroup-per-stream kernels because the workspace is missing
 * or too small to try, it returns hipErrorInvalidValue under the switch and launches nothing.  (The fused PNG kernel has
 * its own switch, DEBIG_FUSED_FLAGS & 2.) */
/* DEBIG_STAGE_GRID (environment variable, read at every call; tests): the launchers below whose kernels loop over their
 * tasks -- debig_hip_apng_composite_batch, debig_hip_png_resize_batch / _resize_alpha / _resize_cubic / _resize_color,
 * _label_gather, _color_label, _warp / _warp_color / _label_warp / _color_label_warp, _persp / _persp_color / _label_persp / _color_label_persp,
 * _elastic / _elastic_color / _label_elastic / _color_label_elastic, _tone_hist / _tone_apply, _blur, _label_stats and
 * _label_boundary, _label_distance_rows / _label_distance_cols -- and the five launchers of the label components,
 * _label_components_rows / _merge / _count / _number / _finish -- and the two of the PNG encode, _png_encode_filter / _png_encode_deflate --
 * and the two of its level 2, _png_encode_dynamic / _png_encode_codes, and the one of its level 3, _png_encode_lz --
 * start min(n_tasks, 2^20) workgroups.  Set to a number G > 0 they start min(G, n_tasks, 2^20), so that a workgroup takes
 * tasks blockIdx.x, blockIdx.x + G, ... one after the other: what a call of more than 2^20 tasks does, at a size a test
 * can afford.  Unset, empty or 0: the launch is unchanged.  Results do not depend on it. */
int debig_hip_inflate_batch_ex(const void *d_in, void *d_out, const debig_stream *d_streams,
                               debig_result *d_results, uint32_t n, uint32_t waves_per_stream,
                               void *hip_stream);

/* One-time set-up of the stream's device: the fixed-Huffman table images every inflate call reads
 * (three small allocations, three tiny kernels, one synchronisation of `hip_stream`).  Calls do it
 * lazily on first use; call it yourself BEFORE capturing a stream into a hipGraph -- allocations and
 * synchronisation are illegal during capture.  Thread safe, idempotent.  0 or a hipError_t. */
int debig_hip_init(void *hip_stream);

/* Concurrency: calls on different streams or from different host threads are safe.  Callers that
 * bring no workspace share ONE cached buffer per device: their groups of launches are serialised
 * on it (each group waits for the event of the group before it), so concurrent callers that want
 * overlap on the device should bring their own workspace.
 *
 * Same with caller-owned workspace for DEBIG_WAVES_SPLIT (no allocation inside the call once
 * debig_hip_init() has run on the device: safe to capture into a hipGraph).
 * debig_hip_inflate_workspace_bytes() is the size that lets ordinary
 * data through the scan/LZ77 pair (about 12 x the compressed bytes of the largest group of 16384
 * streams + 24 KiB per stream); less is legal and only sends more streams down the one-kernel
 * path.  d_workspace = NULL: the internal cached workspace.  The workspace holds no state between
 * calls. */
uint64_t debig_hip_inflate_workspace_bytes(uint64_t total_in_bytes, uint32_t n);
/* The same for a caller that also knows the recipients: total_out_cap = the sum of out_cap.  Highly compressible
 * streams (flat image areas: 30 KB for 4 MB, codes of one or two bits) write many more token units per compressed byte
 * than 12 x allows for; the plan step gives every stream a share by in_len + min(out_cap / 64, 4 in_len) + 2 KiB, and
 * this size adds the second term (at most 3/16 of total_out_cap), so that such streams are not handed back.
 * The other end of the same matter is a SHORT stream of such codes (a run of one byte: 60 KB from 50 bytes of input): one
 * lane decodes all of it, and DEBIG_WAVES_SPLIT / _SPLIT_QUEUED keep a 256-byte token row per symbol of a window's busiest
 * lane.  Below 1 KiB of input the plan step therefore counts the recipient as min(out_cap / 16, 4352), and this size allows
 * every stream for it (it sees sums only): at most 3/4 of total_out_cap and 51 KiB per stream on top.  What this does NOT
 * cover: symbols of one or two bits that produce ONE byte each (a run coded as literals, Z_HUFFMAN_ONLY: 545 rows for 4 KB
 * of input) -- those are handed back.  tests/test_emu_handback.py and tests/test_gpu_handback.py hold the routes to this
 * under DEBIG_NO_HANDBACK. */
uint64_t debig_hip_inflate_workspace_bytes_io(uint64_t total_in_bytes, uint64_t total_out_cap, uint32_t n);
/* workspace that lets DEBIG_WAVES_CHUNKED take every stream of a batch: total_out_bytes = the sum
 * of the recipients (out_cap), which should be close to the decoded sizes */
uint64_t debig_hip_inflate_chunked_workspace_bytes(uint64_t total_in_bytes, uint64_t total_out_bytes, uint32_t n);
int debig_hip_inflate_batch_ws(const void *d_in, void *d_out, const debig_stream *d_streams,
                               debig_result *d_results, uint32_t n, uint32_t waves_per_stream,
                               void *d_workspace, uint64_t workspace_bytes, void *hip_stream);

/* DEBIG_WAVES_SPLIT in two steps, for callers that inflate batches with the SAME descriptors again
 * and again (a decode loop over equal-sized buffers, a captured graph): the share of the workspace
 * every stream gets depends on the descriptors only, so it can be carved once.
 *   debig_hip_inflate_plan_ws     carves `d_workspace` for these n <= 16384 descriptors (one small
 *                                 kernel: what debig_hip_inflate_batch_ws does first on every call);
 *   debig_hip_inflate_planned_ws  scan + LZ77 (+ the one-kernel path for streams handed back) over a
 *                                 workspace that plan_ws carved for exactly these descriptors, this n
 *                                 and this workspace size and that nothing else has written since
 *                                 (the kernels leave the plan intact: call it any number of times).
 * Results are those of debig_hip_inflate_batch_ws.  n > 16384 or no workspace: hipErrorInvalidValue
 * (such batches go through the workspace group by group: use debig_hip_inflate_batch_ws). */
int debig_hip_inflate_plan_ws(const debig_stream *d_streams, uint32_t n, void *d_workspace, uint64_t workspace_bytes,
                              void *hip_stream);
int debig_hip_inflate_planned_ws(const void *d_in, void *d_out, const debig_stream *d_streams, debig_result *d_results,
                                 uint32_t n, void *d_workspace, uint64_t workspace_bytes, void *hip_stream);
/* the same with the dispatch named: DEBIG_WAVES_SPLIT (what debig_hip_inflate_planned_ws runs) or
 * DEBIG_WAVES_SPLIT_QUEUED (persistent workgroups over a work queue: batches whose order mixes cheap and
 * expensive streams); anything else: hipErrorInvalidValue */
int debig_hip_inflate_planned_ws_ex(const void *d_in, void *d_out, const debig_stream *d_streams,
                                    debig_result *d_results, uint32_t n, uint32_t waves_per_stream,
                                    void *d_workspace, uint64_t workspace_bytes, void *hip_stream);

/* One image for the de-filter kernel: the inflated scanline stream (filter byte
 * + w*bpp bytes per row) -> 4-channel RGBA. */
typedef struct debig_png_image {
    uint64_t stream_off; /* inflated stream, relative to d_streams_arena               */
    uint64_t rgba_off;   /* output, relative to d_rgba_arena; 4*w*h bytes              */
    uint64_t pal_off;    /* colour type 3: 768 bytes R[256] G[256] B[256], rel. to d_streams_arena */
    uint32_t width, height;
    uint32_t color_type; /* 6 (RGBA), 3 (palette), 2 (RGB)                                */
    uint32_t asserts_off;/* 0: a filter byte > 4 fails the image (reference default build) */
    /* colour type 2 only: replay_p3 = 1 reproduces the reference's output for RGB images bit
     * for bit (its RGB->RGBA expansion runs inside the row loop): rgba_off
     * must then hold the caller's PRIOR buffer contents and tmp_off a second 4*w*h byte
     * buffer (relative to d_rgba_arena).  replay_p3 = 0: spec-conforming RGB -> RGBA. */
    /* colour type 3 only: rows wider than 16384 pixels need width + 16 bytes of scratch at tmp_off
     * (relative to d_rgba_arena, 4-byte aligned, not 0): the index row handed from one band of 64
     * rows to the next; narrower palette images keep that row in LDS and ignore tmp_off. */
    uint64_t tmp_off;
    uint32_t replay_p3;
    uint32_t reserved;
} debig_png_image;

typedef struct debig_png_result {
    uint32_t good;
    uint32_t bad_row; /* first row whose filter byte was > 4 (when good == 0) */
} debig_png_result;

/* De-filter n inflated scanline streams into RGBA (device pointers, asynchronous on
 * hip_stream).  d_streams_arena must stay readable for 16 bytes past the end of every
 * stream (h * (w * bpp + 1) bytes): rows are fetched as aligned 16-byte pieces.
 * Up to 128 images: an image is spread over 16 / 8 / 4 / 2 workgroups (n <= 16 / 32 / 64 / 128; fewer when the device
 * does not hold them all at once), the bands of 64 rows handed from wavefront to wavefront through memory; images whose
 * workgroups turn out not to be resident together are decoded again by one workgroup inside the same call (never
 * failed).  That mode uses a per-device scratch of progress words shared by the callers of the device (calls are
 * ordered on it by events: such a call cannot be captured into a graph).
 * DEBIG_DEFILTER_NO_REDO (environment variable, read at every call like DEBIG_NO_HANDBACK; tests): set to anything but the
 * empty string or "0", that second launch -- one workgroup per image over the images the several-workgroups launch gave
 * up -- is left out.  An image given up then keeps what the first launch wrote: good = 0, bad_row = 0xfffffffd
 * (PNG_ROW_REDO), pixels unspecified; every other image is the several-workgroups launch's own work, which is what the
 * switch is for: without it nothing in the results says which launch produced the pixels.  Calls that take the
 * one-workgroup kernels from the start (more than 128 images, or a device that does not hold two workgroups per image) do
 * not read it.  debig_hip_png_decode_fused_batch has its own REDO launch and does not read it either. */
int debig_hip_png_defilter_batch(const void *d_streams_arena, void *d_rgba_arena,
                                 const debig_png_image *d_images, debig_png_result *d_results,
                                 uint32_t n, void *hip_stream);

/* SURVEY.md 8(f) row 1 -- inflate AND de-filter n PNG images in ONE kernel launch (debig_png_fused_kernel):
 * replaces the pair src/decode_png.c:800-820 (inflate of the IDAT payload) -> src/decode_png.c:1381-1564 (the row
 * loops over the buffer it filled).  Stream i (d_streams[i]: compressed bytes in d_in, recipient inside
 * d_streams_arena) and image i (d_images[i]: stream_off == d_streams[i].out_off) belong together.  A workgroup owns an
 * image: one wavefront scans the DEFLATE stream, one replays it into the scanline stream, two de-filter bands of 64
 * rows as soon as their bytes are final -- read from L2, where the same CU has just put them; the scanline stream is
 * never read back from HBM, and the de-filter of an image no longer waits for the slowest inflate of the batch.
 * Results are those of debig_hip_inflate_batch_ws (d_results) followed by debig_hip_png_defilter_batch
 * (d_png_results), bit for bit: streams the scan hands back are decoded by debig_inflate_kernel and their images
 * de-filtered by the one-workgroup kernel inside the same call; colour type 2 images with replay_p3 go to the P3
 * kernel as always.  d_workspace / workspace_bytes: as debig_hip_inflate_batch_ws (NULL: the library's own).
 * Meant for hundreds to a few thousand images (a workgroup of four wavefronts and 50 KB of LDS per image). */
int debig_hip_png_decode_fused_batch(const void *d_in, void *d_streams_arena, const debig_stream *d_streams,
                                     debig_result *d_results, void *d_rgba_arena, const debig_png_image *d_images,
                                     debig_png_result *d_png_results, uint32_t n, void *d_workspace,
                                     uint64_t workspace_bytes, void *hip_stream);

/* One task of the general de-filter (csrc/png_spec_kernel.inc, behind debig_png_decode_batch in decode_png.h): one
 * (image, Adam7 pass) sub-image of ANY colour type / bit depth the PNG specification allows -> RGBA8 pixels of the
 * full image at (x0 + x dx, y0 + y dy), or pixels of the format out_fmt (debig_hip_png_spec_defilter_fmt_batch).  A
 * non-interlaced image is one task at (0, 0, 1, 1). */
typedef struct debig_png_spec_task {
    uint64_t stream_off;  /* first filter byte of the sub-image's h * (1 + rowbytes) scanline bytes, rel. to d_arena (>= 16) */
    uint64_t rgba_off;    /* the FULL image's output (img_width * img_height pixels), rel. to d_rgba_arena (16-byte aligned) */
    uint64_t pal_off;     /* colour type 3: 256 RGBA dwords (tRNS alpha folded in), rel. to d_arena (4-byte aligned)     */
    uint64_t scratch_off; /* DEBIG_PNG_SPEC_SCRATCH_BYTES(...) of scratch, rel. to d_arena (16-byte aligned)             */
    uint32_t width, height; /* of the sub-image (w_p, h_p >= 1)                                                          */
    uint32_t img_width;     /* row pitch of the output in pixels                                                         */
    uint32_t x0, y0, dx, dy;
    uint8_t bpp_f;          /* filter unit max(1, channels * depth / 8): 1, 2, 3, 4, 6 or 8                              */
    uint8_t depth, color_type, channels;
    uint16_t key[3];        /* tRNS key (colour type 0: key[0]; 2: RGB), raw samples at full depth                      */
    uint16_t has_key;
    uint16_t n_pal;         /* palette entries; an index >= n_pal fails the task with DEBIG_PNG_SPEC_E_PALETTE           */
    uint16_t out_fmt;       /* output format, resolved (decode_png.h DEBIG_PNG_FMT_*: layout 0..3 | DEBIG_PNG_FMT_16); 0 = RGBA8 */
    uint32_t img_height;    /* planar kernel only: rows of the FULL image (a plane is img_height * img_width samples); else unused */
} debig_png_spec_task;

typedef struct debig_png_spec_result {
    uint32_t status;  /* 0, DEBIG_PNG_SPEC_E_FILTER or DEBIG_PNG_SPEC_E_PALETTE */
    uint32_t bad_row; /* first row of the sub-image whose filter byte is > 4 (E_FILTER) */
} debig_png_spec_result;
enum { DEBIG_PNG_SPEC_E_FILTER = 1, DEBIG_PNG_SPEC_E_PALETTE = 2 };
/* scratch of one task: the ring of de-filtered rows handed from band to band (4 rows of 16-byte groups) */
#define DEBIG_PNG_SPEC_SCRATCH_BYTES(rowbytes) (4u * ((((uint64_t)(rowbytes) + 15u) / 16u) * 16u + 16u))

/* De-filter n tasks (device pointers, asynchronous on hip_stream): one workgroup of four wavefronts per task.  d_arena
 * must stay readable for 16 bytes past the end of every task's scanline bytes (rows are fetched as 16-byte pieces). */
int debig_hip_png_spec_defilter_batch(void *d_arena, void *d_rgba_arena, const debig_png_spec_task *d_tasks,
                                      debig_png_spec_result *d_results, uint32_t n, void *hip_stream);
/* The same for tasks of any output format (each task's out_fmt; 0 is RGBA8, byte for byte as above): pixels of
 * channels * bytes-per-sample bytes, rows of img_width pixels without padding, 16-bit samples little-endian. */
int debig_hip_png_spec_defilter_fmt_batch(void *d_arena, void *d_out_arena, const debig_png_spec_task *d_tasks,
                                          debig_png_spec_result *d_results, uint32_t n, void *hip_stream);
/* The same pixels channel-planar: sample c of pixel (x, y) at rgba_off + (c * img_height * img_width + y * img_width + x) *
 * bytes-per-sample -- planes one after the other, no padding between planes or rows, 16-bit samples little-endian; every
 * task needs img_height.  One-channel formats (GRAY) are the same bytes as above.  Only the image's
 * channels * img_height * img_width * bytes-per-sample bytes are written. */
int debig_hip_png_spec_defilter_planar_batch(void *d_arena, void *d_out_arena, const debig_png_spec_task *d_tasks,
                                             debig_png_spec_result *d_results, uint32_t n, void *hip_stream);

/* The same tasks to raw labels (debig_png_spec_defilter_index_kernel, behind debig_png_decode_batch_labels in decode_png.h):
 * colour types 3 and 0 only (any other task fails as if its filter byte were bad).  One element per pixel at
 * rgba_off + ((y0 + y dy) * img_width + x0 + x dx) * element size: the palette index or the grey sample as stored, one byte
 * for depths up to 8, one little-endian uint16 for depth 16 -- the element size follows from `depth`.  pal_off, key, has_key
 * and out_fmt are not read; an index >= n_pal still fails the task with DEBIG_PNG_SPEC_E_PALETTE. */
int debig_hip_png_spec_defilter_index_batch(void *d_arena, void *d_out_arena, const debig_png_spec_task *d_tasks,
                                            debig_png_spec_result *d_results, uint32_t n, void *hip_stream);

/* APNG compositing (csrc/apng_kernel.inc, behind debig_apng_decode_batch in decode_png.h).  One frame of a file: its
 * RGBA8 pixels (width * height dwords, rows without padding) and its place on the canvas. */
typedef struct debig_apng_frame_desc {
    uint64_t rgba_off;          /* the frame's pixels, rel. to d_frames_arena (4-byte aligned)              */
    uint32_t x_off, y_off;      /* region on the canvas: x_off + width <= canvas width, the same for y      */
    uint32_t width, height;     /* >= 1                                                                      */
    uint8_t dispose_op;         /* 0 NONE, 1 BACKGROUND, 2 PREVIOUS (PREVIOUS on frame 0 acts as BACKGROUND) */
    uint8_t blend_op;           /* 0 SOURCE, 1 OVER                                                          */
    uint16_t reserved;
    uint32_t reserved2;
} debig_apng_frame_desc;

/* One task: pixels [px0, px0 + n_px) of one file's canvas (n_px <= DEBIG_APNG_TASK_PX), through all of its frames. */
typedef struct debig_apng_task {
    uint64_t out_off;           /* the file's output: n_frames canvases of width * height * 4 bytes, rel. to d_out_arena (any alignment) */
    uint64_t ftab_off;          /* the file's n_frames debig_apng_frame_desc, rel. to d_frames_arena (8-byte aligned) */
    uint64_t px0;
    uint32_t n_px;
    uint32_t n_frames;          /* >= 1 */
    uint32_t width, height;     /* the canvas */
} debig_apng_task;
#define DEBIG_APNG_TASK_PX 1024u /* pixels of one task: 256 lanes x 4 consecutive pixels */

/* Composite n tasks (device pointers, asynchronous on hip_stream): one workgroup of 256 lanes per task, each lane a run
 * of 4 consecutive canvas pixels held in registers through the file's frames (the APNG rules of decode_png.h). */
int debig_hip_apng_composite_batch(const void *d_frames_arena, void *d_out_arena, const debig_apng_task *d_tasks,
                                   uint32_t n_tasks, void *hip_stream);

/* Resize + normalise (csrc/png_resize_kernel.inc, behind debig_png_decode_batch_tensor in decode_png.h).  One task: a tile
 * of tile_w x tile_h output pixels (all channels) of one image, one workgroup.  The tile is chosen on the host so that
 * the horizontally filtered rows it needs (src_rows rows of tile_w * channels 16-bit values) fit DEBIG_PNG_RESIZE_HQ_CAP
 * and its slice of the horizontal weights fits DEBIG_PNG_RESIZE_WX_CAP; a task that breaks a bound is skipped. */
typedef struct debig_png_resize_task {
    uint64_t src_off;       /* sample (0, 0) of the CROP, in bytes rel. to d_src_arena (aligned to the sample size)         */
    uint64_t out_off;       /* the image's slot, in bytes rel. to d_out (aligned to the element size)                       */
    uint64_t wx_off, wy_off; /* the axis tables of the crop's width / height, in bytes rel. to d_weights (8-byte aligned)    */
    uint32_t src_pitch;     /* samples from one source row to the next                                                       */
    uint32_t tile_x, tile_y, tile_w, tile_h; /* output pixels; tile_w <= DEBIG_PNG_RESIZE_TILE_W                              */
    uint32_t src_y0, src_rows; /* crop rows [src_y0, src_y0 + src_rows) hold every vertical tap of the tile's rows          */
    uint32_t out_sx, out_sy, out_sc; /* output strides of x, y and the channel, in ELEMENTS (HWC: C, W*C, 1; CHW: 1, W, H*W) */
    uint8_t channels;       /* 1..4, interleaved in the source                                                               */
    uint8_t bits;           /* P: 8 (uint8 samples) or 16 (uint16, little-endian)                                            */
    uint8_t dtype;          /* decode_png.h DEBIG_PNG_T_*: UINT (uint8 for P = 8, uint16 for P = 16), F32, F16, BF16          */
    uint8_t reserved;
    float a[4], b[4];       /* float dtypes: element = (float)v * a[c] + b[c], two rounded operations (decode_png.h)         */
} debig_png_resize_task;
/* An axis table (crop length cl -> L outputs): uint32 max_taps, L; then L pairs of uint32 (first tap, tap count); then
 * L * max_taps int16 Q14 weights, output X's at X * max_taps.  Built on the host by the integer rule of decode_png.h. */
#define DEBIG_PNG_RESIZE_TILE_W 64u
#define DEBIG_PNG_RESIZE_HQ_CAP 12288u /* 16-bit values of one tile's horizontally filtered rows (24 KB of LDS) */
#define DEBIG_PNG_RESIZE_WX_CAP 4096u  /* int16 weights of one tile's columns (8 KB of LDS) */

/* Resize n_tasks tiles (device pointers, asynchronous on hip_stream): pass 1 filters the tile's source rows horizontally
 * into LDS, pass 2 filters them vertically, converts and stores.  Nothing but the tiles' own output elements is written. */
int debig_hip_png_resize_batch(const void *d_src_arena, void *d_out, const debig_png_resize_task *d_tasks,
                               const void *d_weights, uint32_t n_tasks, void *hip_stream);

/* The same with alpha (debig_png_resize_alpha_kernel, behind debig_png_decode_batch_tensor_alpha in decode_png.h): the source
 * is RGBA or GRAY_ALPHA, premultiplied as it is read, filtered premultiplied, and either stored with its alpha
 * (PREMULTIPLIED: out_channels == src_channels) or composited over bg (OVER: out_channels == src_channels - 1).  The first
 * 108 bytes are the fields of debig_png_resize_task with the same meaning; `channels` is the SOURCE channel count (2 or 4,
 * alpha last), the output strides and a[] / b[] are those of the OUTPUT channels.  The tile bounds are the ones above, on
 * the source channel count: src_rows * tile_w * src_channels <= DEBIG_PNG_RESIZE_HQ_CAP; a task that breaks a bound, or
 * whose mode and channel counts do not go together, is skipped. */
typedef struct debig_png_resize_alpha_task {
    uint64_t src_off, out_off, wx_off, wy_off;
    uint32_t src_pitch;     /* SAMPLES from one source row to the next (image width * src_channels)                          */
    uint32_t tile_x, tile_y, tile_w, tile_h;
    uint32_t src_y0, src_rows;
    uint32_t out_sx, out_sy, out_sc; /* in elements of the OUTPUT (HWC: out_channels, W * out_channels, 1; CHW: 1, W, H*W)    */
    uint8_t channels;       /* == src_channels                                                                                */
    uint8_t bits, dtype, reserved;
    float a[4], b[4];       /* indexed by output channel                                                                      */
    uint32_t mode;          /* decode_png.h: DEBIG_PNG_ALPHA_PREMULTIPLIED or _OVER (STRAIGHT is the plain kernel's)          */
    uint8_t src_channels;   /* 4 (R, G, B, A) or 2 (Y, A)                                                                     */
    uint8_t out_channels;   /* OVER: src_channels - 1; PREMULTIPLIED: src_channels                                            */
    uint16_t reserved2;
    uint16_t bg[4];         /* OVER: the background per output channel at precision P, 0 .. 2^P - 1                           */
} debig_png_resize_alpha_task;
int debig_hip_png_resize_alpha_batch(const void *d_src_arena, void *d_out, const debig_png_resize_alpha_task *d_tasks,
                                     const void *d_weights, uint32_t n_tasks, void *hip_stream);

/* The signed filter (debig_png_resize_cubic_kernel, behind debig_png_decode_batch_tensor_filter with DEBIG_PNG_FILTER_BICUBIC
 * in decode_png.h): weights of either sign, signed sums, a biased 16-bit intermediate and the clamps of the header.  The
 * task has the layout of debig_png_resize_alpha_task, field for field, and covers all three alpha modes:
 *   - mode STRAIGHT: 1..4 source channels, out_channels == src_channels, no premultiplication;
 *   - mode PREMULTIPLIED / OVER: as the alpha task (2 or 4 source channels, alpha last).
 * The axis tables, the tile bounds (on the source channel count) and the LDS are those of the kernels above; a task that
 * breaks a bound, or whose mode, channel counts, depth or dtype do not go together, is skipped. */
typedef struct debig_png_resize_cubic_task {
    uint64_t src_off, out_off, wx_off, wy_off;
    uint32_t src_pitch;     /* SAMPLES from one source row to the next (image width * src_channels)                          */
    uint32_t tile_x, tile_y, tile_w, tile_h;
    uint32_t src_y0, src_rows;
    uint32_t out_sx, out_sy, out_sc; /* in elements of the OUTPUT                                                             */
    uint8_t channels;       /* == src_channels                                                                                */
    uint8_t bits, dtype, reserved;
    float a[4], b[4];       /* indexed by output channel                                                                      */
    uint32_t mode;          /* decode_png.h: DEBIG_PNG_ALPHA_STRAIGHT, _PREMULTIPLIED or _OVER                                */
    uint8_t src_channels;   /* STRAIGHT: 1..4; else 4 (R, G, B, A) or 2 (Y, A)                                                */
    uint8_t out_channels;   /* OVER: src_channels - 1; else src_channels                                                      */
    uint16_t reserved2;
    uint16_t bg[4];         /* OVER: the background per output channel at precision P, 0 .. 2^P - 1                           */
} debig_png_resize_cubic_task;
int debig_hip_png_resize_cubic_batch(const void *d_src_arena, void *d_out, const debig_png_resize_cubic_task *d_tasks,
                                     const void *d_weights, uint32_t n_tasks, void *hip_stream);

/* Crop + nearest pick + remap + widening of raw labels (csrc/png_label_kernel.inc, behind debig_png_decode_batch_labels in
 * decode_png.h).  One task: the output rows [row0, row0 + rows) of one image, one workgroup of 256 lanes.  Element (X, Y) of
 * the image is the source label at sy[Y] * src_pitch + sx[X] (counted in labels from src_off), through the call's LUT when it
 * has one, stored as `dtype`.  A task that breaks a bound -- sizes, a table offset that is not a multiple of 16, a dtype of
 * one byte or a LUT with two-byte labels -- is skipped. */
typedef struct debig_png_label_task {
    uint64_t src_off;        /* label (0, 0) of the CROP, in bytes rel. to d_src_arena (aligned to src_bytes)                 */
    uint64_t out_off;        /* the image's slot, in bytes rel. to d_out (aligned to the element size)                        */
    uint64_t sx_off, sy_off; /* out_w / out_h uint32 indices inside the crop, in bytes rel. to d_tables (16-byte aligned)     */
    uint32_t src_pitch;      /* labels from one source row to the next (the image's width)                                    */
    uint32_t out_w, out_h;   /* 1 .. 16384                                                                                    */
    uint32_t row0, rows;     /* row0 + rows <= out_h                                                                          */
    uint8_t src_bytes;       /* 1, or 2 (little-endian uint16)                                                                */
    uint8_t dtype;           /* decode_png.h DEBIG_PNG_L_*: uint8, uint16, int32, int64                                       */
    uint16_t reserved;
} debig_png_label_task;
/* Gather n_tasks row runs (device pointers, asynchronous on hip_stream).  d_lut: 256 int32 in device memory, staged in LDS
 * once per workgroup, or NULL (the element is the label itself; two-byte labels need NULL).  Nothing but the tasks' own
 * output elements is written. */
int debig_hip_png_label_gather_batch(const void *d_src_arena, void *d_out, const debig_png_label_task *d_tasks,
                                     const void *d_tables, const int32_t *d_lut, uint32_t n_tasks, void *hip_stream);

/* Crop + nearest pick + colour pack + colour -> class lookup + widening of decoded RGB8 masks (csrc/png_color_label_kernel.inc,
 * behind debig_png_decode_batch_color_labels in decode_png.h).  Tasks, workgroups and the sx / sy tables are those of the raw-label
 * gather above; the source is interleaved RGB8, three bytes per pixel at any alignment.  Element (X, Y) of the image comes from
 * the pixel at sy[Y] * src_pitch + sx[X] (counted in pixels from src_off), key = R | G << 8 | B << 16:
 *   mode 0 (DEBIG_PNG_CL_PACK): the key itself, dtype int32 or int64;
 *   mode 1 (DEBIG_PNG_CL_MAP):  the value of the key in the task's table, else `missing`; every element that takes `missing`
 *                               adds one to d_unmatched[image].
 * THE TABLE of a colour map of n <= DEBIG_PNG_CMAP_MAX distinct keys, so that a device-pointer caller can build one: `slots`
 * pairs of uint32 (key, value), side by side, 8 bytes per slot, 16-byte aligned in d_tables; slots is a power of two,
 * >= 2 n, >= 2 and <= DEBIG_PNG_CMAP_MAX_SLOTS (the host takes the smallest); an unused slot holds the key
 * DEBIG_PNG_CMAP_EMPTY, which no 24-bit key equals.  A key lives in the first unused slot of the sequence
 * DEBIG_PNG_CMAP_SLOT(key, slots), + 1, + 2, ... (mod slots) at the time it is inserted (linear probing); the value is the
 * int32 as its bits.  A lookup walks that sequence until it finds the key (hit), an unused slot (miss), or has looked at
 * `slots` slots (miss): it terminates on any contents.  The workgroup stages the table in LDS (at most 32 KB), again only when
 * map_off or map_slots differ from the task it did before.
 * A task that breaks a bound -- the sizes and table offsets of the raw-label task, an unknown dtype or mode, PACK with a dtype
 * of one or two bytes, MAP with a slot count that is no power of two, below 2 or above DEBIG_PNG_CMAP_MAX_SLOTS, with a map_off
 * that is no multiple of 16 or without d_unmatched -- is skipped.  src_off, out_off and image are the caller's word, as
 * everywhere in this header. */
#define DEBIG_PNG_CMAP_MAX_SLOTS 4096u
#define DEBIG_PNG_CMAP_EMPTY 0xFFFFFFFFu
#define DEBIG_PNG_CMAP_SLOT(key, slots) ((((uint32_t)(key) * 0x9E3779B1u) >> 20) & ((slots) - 1u))
typedef struct debig_png_color_label_task {
    uint64_t src_off;        /* pixel (0, 0) of the CROP, in bytes rel. to d_src_arena (any alignment)                        */
    uint64_t out_off;        /* the image's slot, in bytes rel. to d_out (aligned to the element size)                        */
    uint64_t sx_off, sy_off; /* out_w / out_h uint32 indices inside the crop, in bytes rel. to d_tables (16-byte aligned)     */
    uint64_t map_off;        /* MAP: the image's table, in bytes rel. to d_tables (16-byte aligned)                           */
    uint32_t src_pitch;      /* pixels from one source row to the next (the image's width)                                    */
    uint32_t out_w, out_h;   /* 1 .. 16384                                                                                    */
    uint32_t row0, rows;     /* row0 + rows <= out_h                                                                          */
    uint32_t map_slots;      /* MAP: slots of the table                                                                       */
    int32_t missing;         /* MAP: the element of a colour that is not in the table                                         */
    uint32_t image;          /* MAP: the image's counter in d_unmatched                                                       */
    uint8_t dtype;           /* decode_png.h DEBIG_PNG_L_*: uint8, uint16, int32, int64                                       */
    uint8_t mode;            /* decode_png.h DEBIG_PNG_CL_*                                                                   */
    uint16_t reserved;
    uint32_t reserved2;
} debig_png_color_label_task;
/* n_tasks row runs (device pointers, asynchronous on hip_stream).  d_unmatched: one uint32 per image, zeroed by the caller;
 * one atomic add per wavefront and task; may be NULL when every task is PACK.  Nothing but the tasks' own output elements and
 * counters is written. */
int debig_hip_png_color_label_batch(const void *d_src_arena, void *d_out, const debig_png_color_label_task *d_tasks,
                                    const void *d_tables, uint32_t *d_unmatched, uint32_t n_tasks, void *hip_stream);

/* Crop + affine warp + normalise of decoded pixels (csrc/png_warp_kernel.inc, behind debig_png_decode_batch_tensor_warp in
 * decode_png.h, which has the rule).  One task: the output rows [row0, row0 + rows) of one image, one workgroup of 256 lanes, one
 * lane per output pixel.  m[] is the image's inverse map as debig_png_warp_quantise gives it (Q16; |m[0]|, |m[1]|, |m[3]|,
 * |m[4]| <= 2^31, |m[2]|, |m[5]| <= 2^40); the pixels are gathered straight from the arena, every tap index clamped into the
 * crop before it addresses memory.  A task that breaks a bound -- the sizes (out_w, out_h 1 .. 16384, row0 + rows <= out_h,
 * crop_w, crop_h 1 .. 2^31 - 1), channels outside 1 .. 4, bits other than 8 / 16, an unknown dtype, filter or border mode, a
 * matrix entry beyond its limit, a src_off that is not aligned to the sample size -- is skipped. */
typedef struct debig_png_warp_task {
    uint64_t src_off;       /* sample (0, 0) of the CROP, in bytes rel. to d_src_arena (aligned to the sample size)         */
    uint64_t out_off;       /* the image's slot, in bytes rel. to d_out (aligned to the element size)                       */
    int64_t m[6];           /* the inverse map, row major, Q16                                                               */
    uint32_t src_pitch;     /* samples from one source row to the next (image width * channels)                              */
    uint32_t crop_w, crop_h; /* the crop in pixels: taps outside [0, crop_w) x [0, crop_h) are border                        */
    uint32_t out_w, out_h;  /* 1 .. 16384                                                                                    */
    uint32_t row0, rows;    /* row0 + rows <= out_h                                                                          */
    uint32_t out_sx, out_sy, out_sc; /* output strides of x, y and the channel, in ELEMENTS (HWC: C, W*C, 1; CHW: 1, W, H*W) */
    uint8_t channels;       /* 1..4, interleaved in the source                                                               */
    uint8_t bits;           /* P: 8 (uint8 samples) or 16 (uint16, little-endian)                                            */
    uint8_t dtype;          /* decode_png.h DEBIG_PNG_T_*                                                                    */
    uint8_t filter;         /* decode_png.h DEBIG_PNG_FILTER_BILINEAR or _NEAREST                                            */
    uint8_t border_mode;    /* decode_png.h DEBIG_PNG_BORDER_CONSTANT or _CLAMP                                              */
    uint8_t reserved[3];
    uint16_t border[4];     /* CONSTANT: the border sample per channel at precision P, 0 .. 2^P - 1                          */
    float a[4], b[4];       /* float dtypes: element = (float)v * a[c] + b[c], two rounded operations (decode_png.h)         */
} debig_png_warp_task;
/* Warp n_tasks row runs (device pointers, asynchronous on hip_stream).  Nothing but the tasks' own output elements is written. */
int debig_hip_png_warp_batch(const void *d_src_arena, void *d_out, const debig_png_warp_task *d_tasks, uint32_t n_tasks,
                             void *hip_stream);

/* The same warp of raw labels (debig_png_label_warp_kernel, behind debig_png_decode_batch_labels_warp in decode_png.h): nearest
 * only, the pick of the image task's NEAREST filter under the same m[].  The source is one byte or one little-endian uint16 per
 * pixel; the element is the label, through the call's LUT when it has one, or border_label AS IT IS where the pick leaves the
 * crop under CONSTANT; stored as `dtype`.  A task that breaks a bound -- the sizes and matrix limits above, src_bytes other than
 * 1 / 2, an unknown dtype or border mode, a dtype of one byte or a LUT with two-byte labels, a src_off that is not aligned to
 * src_bytes -- is skipped. */
typedef struct debig_png_label_warp_task {
    uint64_t src_off;        /* label (0, 0) of the CROP, in bytes rel. to d_src_arena (aligned to src_bytes)                 */
    uint64_t out_off;        /* the image's slot, in bytes rel. to d_out (aligned to the element size)                        */
    int64_t m[6];            /* the inverse map, row major, Q16                                                               */
    uint32_t src_pitch;      /* labels from one source row to the next (the image's width)                                    */
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;   /* 1 .. 16384                                                                                    */
    uint32_t row0, rows;     /* row0 + rows <= out_h                                                                          */
    int32_t border_label;    /* CONSTANT: the element of a pick outside the crop (inside the dtype's range)                   */
    uint8_t src_bytes;       /* 1, or 2 (little-endian uint16)                                                                */
    uint8_t dtype;           /* decode_png.h DEBIG_PNG_L_*: uint8, uint16, int32, int64                                       */
    uint8_t border_mode;     /* decode_png.h DEBIG_PNG_BORDER_CONSTANT or _CLAMP                                              */
    uint8_t reserved;
    uint32_t reserved2;
} debig_png_label_warp_task;
/* n_tasks row runs (device pointers, asynchronous on hip_stream).  d_lut: 256 int32 in device memory, staged in LDS once per
 * workgroup, or NULL.  Nothing but the tasks' own output elements is written. */
int debig_hip_png_label_warp_batch(const void *d_src_arena, void *d_out, const debig_png_label_warp_task *d_tasks,
                                   const int32_t *d_lut, uint32_t n_tasks, void *hip_stream);

/* The same warp of colour-coded masks (debig_png_color_label_warp_kernel in csrc/png_color_label_warp_kernel.inc, behind
 * debig_png_decode_batch_color_labels_warp in decode_png.h): tasks, workgroups, m[] and the pick are those of the label warp
 * above; the source, the key, the two modes, THE TABLE and the counters are those of debig_png_color_label_task, unchanged.
 * The picked pixel is three bytes at src_off + (jy * src_pitch + jx) * 3, both indices clamped into the crop first; an element
 * whose pick leaves the crop under CONSTANT is border_label AS IT IS: it does not pass through the table and is never counted
 * in d_unmatched[image], even where border_label == missing.  A clamped pick goes through the table and is counted like any
 * other.  A task that breaks a bound -- the sizes and matrix limits of the warp tasks, an unknown dtype, mode or border mode,
 * PACK with a dtype of one or two bytes, MAP with a slot count that is no power of two, below 2 or above
 * DEBIG_PNG_CMAP_MAX_SLOTS, with a map_off that is no multiple of 16 or without d_unmatched -- is skipped. */
typedef struct debig_png_color_label_warp_task {
    uint64_t src_off;        /* pixel (0, 0) of the CROP, in bytes rel. to d_src_arena (any alignment)                        */
    uint64_t out_off;        /* the image's slot, in bytes rel. to d_out (aligned to the element size)                        */
    uint64_t map_off;        /* MAP: the image's table, in bytes rel. to d_tables (16-byte aligned)                           */
    int64_t m[6];            /* the inverse map, row major, Q16                                                               */
    uint32_t src_pitch;      /* pixels from one source row to the next (the image's width)                                    */
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;   /* 1 .. 16384                                                                                    */
    uint32_t row0, rows;     /* row0 + rows <= out_h                                                                          */
    int32_t border_label;    /* CONSTANT: the element of a pick outside the crop (inside the dtype's range)                   */
    uint32_t map_slots;      /* MAP: slots of the table                                                                       */
    int32_t missing;         /* MAP: the element of a colour that is not in the table                                         */
    uint32_t image;          /* MAP: the image's counter in d_unmatched                                                       */
    uint8_t dtype;           /* decode_png.h DEBIG_PNG_L_*: uint8, uint16, int32, int64                                       */
    uint8_t mode;            /* decode_png.h DEBIG_PNG_CL_*                                                                   */
    uint8_t border_mode;     /* decode_png.h DEBIG_PNG_BORDER_CONSTANT or _CLAMP                                              */
    uint8_t reserved;
} debig_png_color_label_warp_task;
/* n_tasks row runs (device pointers, asynchronous on hip_stream).  d_tables holds the tasks' tables; d_unmatched: one uint32
 * per image, zeroed by the caller; one atomic add per wavefront and task; may be NULL when every task is PACK.  Nothing but
 * the tasks' own output elements and counters is written. */
int debig_hip_png_color_label_warp_batch(const void *d_src_arena, void *d_out, const debig_png_color_label_warp_task *d_tasks,
                                         const void *d_tables, uint32_t *d_unmatched, uint32_t n_tasks, void *hip_stream);

/* ---- the per-image colour matrix of the tensor decodes (csrc/png_color_kernel.inc, behind debig_png_decode_batch_tensor_color and
 * debig_png_decode_batch_tensor_warp_color in decode_png.h, which has the rule).  One RECORD per image, 64 bytes, 8-byte aligned in
 * d_weights: the matrix as debig_png_color_quantise gives it -- k[3 c + j] = llround(m_cj * 65536), |k| <= 2^20; o[c] =
 * llround(m_c3 * Vmax), |o| <= 16 Vmax, Vmax = (2^P - 1) << (30 - P).  It is uniform over a task, so it arrives by scalar loads and
 * the tasks stay small.  A task whose record breaks a limit, or whose color_off is not a multiple of 8, is skipped. */
typedef struct debig_png_color_rec {
    int64_t o[3];
    int32_t k[9];           /* row major: output channel c takes k[3 c .. 3 c + 2]                                           */
    uint32_t reserved;
} debig_png_color_rec;

/* Resize + colour matrix + normalise (debig_png_resize_color_kernel): the tile, the axis tables, the bounds and pass 1 are those of
 * debig_png_resize_task, whose fields come first with the same meaning; channels is 3 (RGB) or 4 (RGBA: the fourth channel is
 * not mixed).  Pass 2 takes an output PIXEL per lane: it sums the channels down the Hq rows, mixes the three colours, converts
 * and stores.  A task that breaks a bound of debig_png_resize_task, or with other channels, bits other than 8 / 16 or an unknown
 * dtype, is skipped. */
typedef struct debig_png_resize_color_task {
    uint64_t src_off, out_off, wx_off, wy_off;
    uint32_t src_pitch;
    uint32_t tile_x, tile_y, tile_w, tile_h;
    uint32_t src_y0, src_rows;
    uint32_t out_sx, out_sy, out_sc;
    uint8_t channels;       /* 3 or 4                                                                                         */
    uint8_t bits, dtype, reserved;
    float a[4], b[4];
    uint32_t reserved2;
    uint64_t color_off;     /* the image's debig_png_color_rec, in bytes rel. to d_weights (8-byte aligned)                   */
} debig_png_resize_color_task;
int debig_hip_png_resize_color_batch(const void *d_src_arena, void *d_out, const debig_png_resize_color_task *d_tasks,
                                     const void *d_weights, uint32_t n_tasks, void *hip_stream);

/* Warp + colour matrix + normalise (debig_png_warp_color_kernel): debig_png_warp_task, field for field, and the image's record.
 * Picks, border rule and clamps are the warp kernel's; a CONSTANT border sample is mixed like any other.  d_weights holds the
 * records (nothing else is read from it). */
typedef struct debig_png_warp_color_task {
    uint64_t src_off, out_off;
    int64_t m[6];
    uint32_t src_pitch;
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;
    uint32_t row0, rows;
    uint32_t out_sx, out_sy, out_sc;
    uint8_t channels;       /* 3 or 4                                                                                         */
    uint8_t bits, dtype, filter, border_mode;
    uint8_t reserved[3];
    uint16_t border[4];
    float a[4], b[4];
    uint64_t color_off;     /* the image's debig_png_color_rec, in bytes rel. to d_weights (8-byte aligned)                   */
} debig_png_warp_color_task;
int debig_hip_png_warp_color_batch(const void *d_src_arena, void *d_out, const debig_png_warp_color_task *d_tasks,
                                   const void *d_weights, uint32_t n_tasks, void *hip_stream);

/* ---- the four warp kernels under a projective map (csrc/png_persp_kernel.inc, behind debig_png_decode_batch_tensor_persp,
 * _labels_persp and _color_labels_persp in decode_png.h, which has the rule).  Each task is the warp task of the kernel it
 * mirrors, field for field, followed by p[]: row 2 of the inverse map as debig_png_persp_quantise gives it (Q30, |p[k]| <= 2^32).
 * m[] holds rows 0 and 1, with the limits of the warp tasks.  Per output pixel D = p[0] cx + p[1] cy + 2 p[2] (Q31) and
 * (U, V) = (floor(NU 2^31 / D), floor(NV 2^31 / D)), NU and NV being the affine U and V of m[]; everything behind (U, V), the
 * tasks' rows, the workgroups, the lane mapping, the buffers and the grid rule are those of the warp launcher of the same kind.
 * A task is skipped when it breaks a bound of its warp counterpart, when a |p[k]| exceeds 2^32, or when D leaves
 * [2^21, 2^33 - 1] at one of the four corner pixels of the out_w x out_h output (D is linear, so that covers every pixel). */
typedef struct debig_png_persp_task {
    uint64_t src_off, out_off;
    int64_t m[6];
    uint32_t src_pitch;
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;
    uint32_t row0, rows;
    uint32_t out_sx, out_sy, out_sc;
    uint8_t channels;       /* 1..4                                                                                           */
    uint8_t bits, dtype, filter, border_mode;
    uint8_t reserved[3];
    uint16_t border[4];
    float a[4], b[4];
    int64_t p[3];           /* row 2 of the inverse map, Q30                                                                  */
} debig_png_persp_task;
int debig_hip_png_persp_batch(const void *d_src_arena, void *d_out, const debig_png_persp_task *d_tasks, uint32_t n_tasks,
                              void *hip_stream);

typedef struct debig_png_persp_color_task {
    uint64_t src_off, out_off;
    int64_t m[6];
    uint32_t src_pitch;
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;
    uint32_t row0, rows;
    uint32_t out_sx, out_sy, out_sc;
    uint8_t channels;       /* 3 or 4                                                                                         */
    uint8_t bits, dtype, filter, border_mode;
    uint8_t reserved[3];
    uint16_t border[4];
    float a[4], b[4];
    uint64_t color_off;
    int64_t p[3];
} debig_png_persp_color_task;
int debig_hip_png_persp_color_batch(const void *d_src_arena, void *d_out, const debig_png_persp_color_task *d_tasks,
                                    const void *d_weights, uint32_t n_tasks, void *hip_stream);

typedef struct debig_png_label_persp_task {
    uint64_t src_off, out_off;
    int64_t m[6];
    uint32_t src_pitch;
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;
    uint32_t row0, rows;
    int32_t border_label;
    uint8_t src_bytes, dtype, border_mode, reserved;
    uint32_t reserved2;
    int64_t p[3];
} debig_png_label_persp_task;
int debig_hip_png_label_persp_batch(const void *d_src_arena, void *d_out, const debig_png_label_persp_task *d_tasks,
                                    const int32_t *d_lut, uint32_t n_tasks, void *hip_stream);

typedef struct debig_png_color_label_persp_task {
    uint64_t src_off, out_off, map_off;
    int64_t m[6];
    uint32_t src_pitch;
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;
    uint32_t row0, rows;
    int32_t border_label;
    uint32_t map_slots;
    int32_t missing;
    uint32_t image;
    uint8_t dtype, mode, border_mode, reserved;
    int64_t p[3];
} debig_png_color_label_persp_task;
int debig_hip_png_color_label_persp_batch(const void *d_src_arena, void *d_out, const debig_png_color_label_persp_task *d_tasks,
                                          const void *d_tables, uint32_t *d_unmatched, uint32_t n_tasks, void *hip_stream);

/* ---- the four warp kernels under an elastic deformation (csrc/png_elastic_kernel.inc, behind
 * debig_png_decode_batch_tensor_elastic, _labels_elastic and _color_labels_elastic in decode_png.h, which has the rule).  Each task
 * is the warp task of the kernel it mirrors, field for field, followed by field_off and the grid size.  field_off: where the
 * task's grid_h x grid_w nodes lie, in bytes from d_fields, a multiple of 8; a node is two int32 (dx, dy) as
 * debig_png_elastic_quantise gives them (Q16, at most 2^28 in magnitude), the grid row major.  UINT64_MAX: no field (d_fields is
 * then not read for the task: it takes a field of zeros and gives the bytes of its warp twin).  Per output pixel the displacement
 * (Dx, Dy) is interpolated from the grid, which the workgroup holds in LDS while consecutive tasks name the same field_off and
 * grid size, and (U, V) = (NU, NV) + the linear part of m[] applied to (Dx, Dy); everything behind (U, V), the tasks' rows, the
 * workgroups, the lane mapping, the other buffers and the grid rule are those of the warp launcher of the same kind.  A task is
 * skipped when it breaks a bound of its warp counterpart, when grid_w or grid_h lies outside 2 .. 33, when field_off is
 * misaligned, or when one of its nodes exceeds 2^28 in magnitude. */
typedef struct debig_png_elastic_task {
    uint64_t src_off, out_off;
    int64_t m[6];
    uint32_t src_pitch;
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;
    uint32_t row0, rows;
    uint32_t out_sx, out_sy, out_sc;
    uint8_t channels;       /* 1..4                                                                                           */
    uint8_t bits, dtype, filter, border_mode;
    uint8_t reserved[3];
    uint16_t border[4];
    float a[4], b[4];
    uint64_t field_off;     /* bytes from d_fields, 8-byte aligned; UINT64_MAX: no field                                      */
    uint16_t grid_w, grid_h; /* 2 .. 33                                                                                       */
    uint32_t reserved3;
} debig_png_elastic_task;
int debig_hip_png_elastic_batch(const void *d_src_arena, void *d_out, const debig_png_elastic_task *d_tasks, const void *d_fields,
                                uint32_t n_tasks, void *hip_stream);

typedef struct debig_png_elastic_color_task {
    uint64_t src_off, out_off;
    int64_t m[6];
    uint32_t src_pitch;
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;
    uint32_t row0, rows;
    uint32_t out_sx, out_sy, out_sc;
    uint8_t channels;       /* 3 or 4                                                                                         */
    uint8_t bits, dtype, filter, border_mode;
    uint8_t reserved[3];
    uint16_t border[4];
    float a[4], b[4];
    uint64_t color_off;
    uint64_t field_off;
    uint16_t grid_w, grid_h;
    uint32_t reserved3;
} debig_png_elastic_color_task;
int debig_hip_png_elastic_color_batch(const void *d_src_arena, void *d_out, const debig_png_elastic_color_task *d_tasks,
                                      const void *d_weights, const void *d_fields, uint32_t n_tasks, void *hip_stream);

typedef struct debig_png_label_elastic_task {
    uint64_t src_off, out_off;
    int64_t m[6];
    uint32_t src_pitch;
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;
    uint32_t row0, rows;
    int32_t border_label;
    uint8_t src_bytes, dtype, border_mode, reserved;
    uint32_t reserved2;
    uint64_t field_off;
    uint16_t grid_w, grid_h;
    uint32_t reserved3;
} debig_png_label_elastic_task;
int debig_hip_png_label_elastic_batch(const void *d_src_arena, void *d_out, const debig_png_label_elastic_task *d_tasks,
                                      const int32_t *d_lut, const void *d_fields, uint32_t n_tasks, void *hip_stream);

typedef struct debig_png_color_label_elastic_task {
    uint64_t src_off, out_off, map_off;
    int64_t m[6];
    uint32_t src_pitch;
    uint32_t crop_w, crop_h;
    uint32_t out_w, out_h;
    uint32_t row0, rows;
    int32_t border_label;
    uint32_t map_slots;
    int32_t missing;
    uint32_t image;
    uint8_t dtype, mode, border_mode, reserved;
    uint64_t field_off;
    uint16_t grid_w, grid_h;
    uint32_t reserved3;
} debig_png_color_label_elastic_task;
int debig_hip_png_color_label_elastic_batch(const void *d_src_arena, void *d_out, const debig_png_color_label_elastic_task *d_tasks,
                                            const void *d_tables, uint32_t *d_unmatched, const void *d_fields, uint32_t n_tasks,
                                            void *hip_stream);

/* ---- tone curves of the tensor decodes (csrc/png_tone_kernel.inc, behind debig_png_decode_batch_tensor_tone in decode_png.h,
 * which has the rule).  The first stage writes every tone file as UINT8 HWC into an arena; one TASK of both kernels is a run of
 * pix_n pixels of one such image, row major from pixel pix0, for one workgroup of 256 lanes.  The histogram kernel takes the tasks
 * of AUTOCONTRAST / EQUALIZE files and adds the counts of the run's colour samples to the image's colour_channels x 256 uint32 at
 * hist_off in d_hist (cleared by the caller before the launch).  The apply kernel takes the tasks of every tone file: it builds
 * the image's tables from that histogram (AUTOCONTRAST, EQUALIZE: d_hist may be NULL when no task needs it) or copies the 256
 * bytes at lut_off in d_tables (every other op: one table for every colour channel), maps the run's colour samples, passes alpha
 * through and stores a[c] * (float)(entry << 22) + b[c] as dtype at out_off + (X out_sx + Y out_sy + c out_sc) elements.
 * A task is skipped when out_w or out_h is 0 or above 16384, pix_n is 0 or above DEBIG_PNG_TONE_MAX_RUN, the run leaves the image,
 * channels is not 1..4, colour_channels is not channels (1, 3) or channels - 1 (2, 4), dtype is above 3, op is not 1..5, hist_off
 * or lut_off is not a multiple of 16, or src_off is not a multiple of a 2- or 4-byte pixel; the histogram kernel also skips the
 * tasks of other ops. */
#define DEBIG_PNG_TONE_RUN 4096u      /* pixels of a task as the host cuts them (the warp kernels' unit)                       */
#define DEBIG_PNG_TONE_MAX_RUN 65536u
typedef struct debig_png_tone_task {
    uint64_t src_off;       /* the image's first pixel, in bytes rel. to d_src                                                 */
    uint64_t out_off;       /* the image's slot, in bytes rel. to d_out                                                        */
    uint64_t hist_off;      /* the image's histograms, in bytes rel. to d_hist                                                 */
    uint64_t lut_off;       /* the image's 256-byte table, in bytes rel. to d_tables                                           */
    uint32_t pix0, pix_n;
    uint32_t out_w, out_h;
    uint32_t out_sx, out_sy, out_sc; /* in elements                                                                            */
    uint8_t channels, colour_channels;
    uint8_t dtype;          /* DEBIG_PNG_T_*                                                                                   */
    uint8_t op;             /* DEBIG_PNG_TONE_* (never NONE)                                                                   */
    float a[4], b[4];
} debig_png_tone_task;
int debig_hip_png_tone_hist_batch(const void *d_src, uint32_t *d_hist, const debig_png_tone_task *d_tasks, uint32_t n_tasks,
                                  void *hip_stream);
int debig_hip_png_tone_apply_batch(const void *d_src, void *d_out, const debig_png_tone_task *d_tasks, const uint32_t *d_hist,
                                   const void *d_tables, uint32_t n_tasks, void *hip_stream);

/* ---- Gaussian blur and sharpness of the tensor decodes (csrc/png_blur_kernel.inc, behind debig_png_decode_batch_tensor_blur in
 * decode_png.h, which has the rule).  The stages in front (a resize or warp kernel, then the tone apply kernel where the file has
 * a tone operation too) have written every blur file as UINT8 HWC into an arena; one TASK is a tile of tile_w x tile_h output
 * pixels at (x0, y0) of one such image of w x h pixels, for one workgroup of 256 lanes.  The workgroup brings the tile and a halo
 * of `radius` pixels on every side (indices folded by the mirror rule) into LDS as bytes, runs the horizontal pass into a 16-bit
 * LDS plane and the vertical pass out of it (GAUSSIAN: the 63 int16 weights at table_off in d_tables, of which 2 radius + 1 are
 * used), or takes the 3 x 3 SMOOTH and the blend with K = k from the byte tile (SHARPNESS), and stores
 * a[c] * (float)v + b[c] as dtype at out_off + (X out_sx + Y out_sy + c out_sc) elements.
 * A task is skipped whole when w or h is 0 or above 16384, the tile is empty, wider or taller than DEBIG_PNG_BLUR_MAX_TILE or
 * leaves the image, channels is not 1..4, colour_channels is not channels (1, 3) or channels - 1 (2, 4), dtype is above 3, op is
 * not 1..2, radius is not 1..31 (GAUSSIAN) or not 1 (SHARPNESS), |k| is above 16 * 65536, (tile_h + 2 radius) x (tile_w + 2 radius)
 * x channels is above DEBIG_PNG_BLUR_PX_CAP, (tile_h + 2 radius) x tile_w x channels is above DEBIG_PNG_BLUR_H16_CAP (GAUSSIAN),
 * table_off is not a multiple of 16, or src_off is not a multiple of a 2- or 4-byte pixel. */
#define DEBIG_PNG_BLUR_TILE 32u       /* the tile edge at which every radius and channel count fits                            */
#define DEBIG_PNG_BLUR_MAX_TILE 64u
#define DEBIG_PNG_BLUR_PX_CAP 35840u  /* bytes of the tile with its halo: (32 + 62)^2 x 4 = 35,344                             */
#define DEBIG_PNG_BLUR_H16_CAP 12288u /* halfwords of the horizontal pass: (32 + 62) x 32 x 4 = 12,032                         */
typedef struct debig_png_blur_task {
    uint64_t src_off;       /* the image's first pixel, in bytes rel. to d_src                                                 */
    uint64_t out_off;       /* the image's slot, in bytes rel. to d_out                                                        */
    uint64_t table_off;     /* GAUSSIAN: the file's 63 int16 weights, in bytes rel. to d_tables                                */
    int32_t k;              /* SHARPNESS: llround(factor * 65536)                                                              */
    uint32_t radius;        /* GAUSSIAN: ksize / 2; SHARPNESS: 1                                                               */
    uint32_t w, h;          /* the image                                                                                       */
    uint32_t x0, y0, tile_w, tile_h;
    uint32_t out_sx, out_sy, out_sc; /* in elements                                                                            */
    uint8_t channels, colour_channels;
    uint8_t dtype;          /* DEBIG_PNG_T_*                                                                                   */
    uint8_t op;             /* DEBIG_PNG_BLUR_* (never NONE)                                                                   */
    float a[4], b[4];
} debig_png_blur_task;
int debig_hip_png_blur_batch(const void *d_src, void *d_out, const debig_png_blur_task *d_tasks, const void *d_tables,
                             uint32_t n_tasks, void *hip_stream);

/* ---- per-id pixel counts and bounding boxes of a dense label tensor (csrc/png_label_stats_kernel.inc, behind
 * debig_png_label_stats in decode_png.h, which has the rule).  An image of out_w x out_h elements has n_ids + 1 RAW records, 20
 * bytes each, at stat_off in d_stats: record k < n_ids for the elements equal to k, record n_ids ("other") for every element that
 * is negative or >= n_ids (an int64 is compared whole: 2^32 + 3 is "other", not 3).  Every field of a raw record only grows, by an
 * add or a max, and all zeros is the empty record: the caller clears d_stats before the launch, no kernel initialises it, and a
 * second launch over other rows of the image accumulates into the same records.  One TASK is a run of whole rows of one image,
 * contiguous in the dense tensor, for one workgroup of 256 lanes; integer adds and maxima commute, so the records do not depend on
 * the grid, the order of the tasks or where the runs are cut.
 * A task is skipped when dtype is above 3, n_ids is 0 or above DEBIG_PNG_LABEL_STATS_MAX_IDS, out_w or out_h is 0 or above 16384,
 * rows is 0 or row0 + rows exceeds out_h, stat_off is not a multiple of 4, or label_off is not a multiple of the element size. */
#define DEBIG_PNG_LABEL_STATS_MAX_IDS 1024u
#define DEBIG_PNG_LABEL_STATS_RUN 16384u /* elements of a task as the host cuts them (the gather kernels' unit)                   */
typedef struct debig_png_label_stat {
    uint32_t count;         /* elements of the id                                                                              */
    uint32_t x_end;         /* max x + 1                                                                                       */
    uint32_t y_end;         /* max y + 1                                                                                       */
    uint32_t x_rev;         /* out_w - min x                                                                                   */
    uint32_t y_rev;         /* out_h - min y                                                                                   */
} debig_png_label_stat;
typedef struct debig_png_label_stats_task {
    uint64_t label_off;     /* the run's first element (row row0, x 0), in bytes rel. to d_labels                              */
    uint64_t stat_off;      /* the image's n_ids + 1 raw records, in bytes rel. to d_stats                                     */
    uint32_t out_w, out_h;  /* the image                                                                                       */
    uint32_t row0, rows;    /* the run                                                                                         */
    uint32_t n_ids;
    uint32_t dtype;         /* decode_png.h DEBIG_PNG_L_*: uint8, uint16, int32, int64                                         */
} debig_png_label_stats_task;
int debig_hip_png_label_stats_batch(const void *d_labels, void *d_stats, const debig_png_label_stats_task *d_tasks, uint32_t n_tasks,
                                    void *hip_stream);

/* ---- boundary bands of a dense label tensor: ignore rings and edge maps (csrc/png_label_boundary_kernel.inc, behind
 * debig_png_label_boundary in decode_png.h, which has the rule).  Element (x, y) of an image of w x h elements is a BOUNDARY element
 * iff an element at (x + dx, y + dy) with |dy| <= radius, |dx| <= reach[|dy|], inside the image, differs from it (elements are
 * compared whole).  mode 0 (RING) writes `boundary ? value : the element` in the dtype of the input, mode 1 (EDGE) one byte 1 / 0.
 * One TASK is a tile of one image for one workgroup of 256 lanes, which stages the tile and a halo of `radius` elements in LDS:
 * the output is a pure function of the input, whatever the tiling, the grid and the order of the tasks.  d_out must not overlap
 * d_labels (a tile reads what its neighbours write).  The kernel takes the reach table as it is and knows nothing about shapes.
 * A task is skipped when dtype is above 3, mode above 1, radius 0 or above DEBIG_PNG_LABEL_BOUNDARY_MAX_RADIUS, a reach entry
 * 0 .. radius exceeds the radius, w or h is 0 or above 16384, tile_w or tile_h is 0 or above DEBIG_PNG_LABEL_BOUNDARY_MAX_TILE or
 * the tile leaves the image, the two staged planes exceed DEBIG_PNG_LABEL_BOUNDARY_LDS_BYTES (DEBIG_PNG_LABEL_BOUNDARY_TILE_BYTES
 * of the largest window; a tile of 32 x 32 fits for every dtype and radius), `value` is outside the dtype under RING, or an offset
 * or address is not a multiple of the element size (of 1 for the output of EDGE). */
#define DEBIG_PNG_LABEL_BOUNDARY_MAX_RADIUS 16u
#define DEBIG_PNG_LABEL_BOUNDARY_MAX_TILE 128u      /* columns and rows of a tile                                                */
#define DEBIG_PNG_LABEL_BOUNDARY_LDS_BYTES 40960u   /* the value plane and the dist plane of one task                            */
typedef struct debig_png_label_boundary_task {
    uint64_t label_off;     /* the image's first element, in bytes rel. to d_labels                                            */
    uint64_t out_off;       /* the image's first output element, in bytes rel. to d_out                                        */
    int64_t value;          /* RING: what a boundary element becomes                                                           */
    uint32_t w, h;          /* the image                                                                                       */
    uint32_t x0, y0, tile_w, tile_h; /* the tile                                                                               */
    uint32_t dtype;         /* decode_png.h DEBIG_PNG_L_*: uint8, uint16, int32, int64                                         */
    uint32_t mode;          /* 0 RING, 1 EDGE                                                                                  */
    uint32_t radius;        /* 1 .. 16                                                                                         */
    uint8_t reach[17];      /* reach[d], d = 0 .. radius: the half-width of the window at a row distance of d                  */
    uint8_t reserved[3];
} debig_png_label_boundary_task;
/* the LDS bytes a tile of tile_w x tile_h elements of 1 << dtype bytes takes at most (a window that no image edge clips):
 * rows x (pitch + dpitch), pitch = ((tile_w + 2 radius) * es + 30) & ~15, dpitch = (pitch / es + 15) & ~15 */
#define DEBIG_PNG_LABEL_BOUNDARY_TILE_BYTES(tile_w, tile_h, dtype, radius)                                                         \
    (((tile_h) + 2u * (radius)) *                                                                                                  \
     ((((((tile_w) + 2u * (radius)) << (dtype)) + 30u) & ~15u) +                                                                   \
      ((((((((tile_w) + 2u * (radius)) << (dtype)) + 30u) & ~15u) >> (dtype)) + 15u) & ~15u)))
int debig_hip_png_label_boundary_batch(const void *d_labels, void *d_out, const debig_png_label_boundary_task *d_tasks, uint32_t n_tasks,
                                       void *hip_stream);

/* ---- exact squared Euclidean distance maps of a dense label tensor (csrc/png_label_distance_kernel.inc, behind
 * debig_png_label_distance in decode_png.h, which has the rule), in two launches on one stream:
 *   ROWS  reads the labels and writes the G PLANE d_g, one uint16 per element of the image (w x h, dense): bits 0 .. 14 the distance
 *         along the row to the nearest site of the element in its row (0 .. 16383, or 0x7fff: none), bit 15 "differs from the
 *         element above" (sites 0 only, never in row 0).  One TASK is a run of whole rows of one image for one workgroup of 256
 *         lanes: rows x w <= DEBIG_PNG_LABEL_DISTANCE_ROWS_ELEMS, or one row.
 *   COLS  reads the g plane and writes the output plane d_out, 4 bytes per element (int32 under format 0, float32 under format 1).
 *         One TASK is a strip of 1 .. DEBIG_PNG_LABEL_DISTANCE_COLS adjacent columns of one image for one wavefront, one lane per
 *         column.  WHILE IT RUNS, A COLUMN'S OUTPUT ELEMENTS HOLD ITS ENVELOPE STACK; every element of the strip is written last
 *         with its result.  It never reads the labels.
 * Both are pure functions of their input, whatever the cut, the grid and the order of the tasks; both do work linear in the row /
 * column length whatever the data.  d_g must not overlap d_labels or d_out.
 * A rows task is skipped when dtype is above 3, sites above 1, w or h is 0 or above 16384, rows is 0 or the run leaves the image,
 * rows x w exceeds the cap with rows above 1, or an offset or address is not a multiple of the element size (of 2 for the g plane);
 * a cols task when format is above 1, cap above 32767, w or h is 0 or above 16384, cols is 0 or above the cap or the strip leaves
 * the image, or an offset or address is not a multiple of 2 (g) / 4 (output). */
#define DEBIG_PNG_LABEL_DISTANCE_ROWS_ELEMS 16384u
#define DEBIG_PNG_LABEL_DISTANCE_COLS 64u
typedef struct debig_png_label_distance_rows_task {
    uint64_t label_off;     /* the image's first element, in bytes rel. to d_labels                                            */
    uint64_t g_off;         /* the image's first g element, in bytes rel. to d_g                                               */
    int64_t value;          /* sites 1: the elements equal to it are the sites (a value the dtype cannot hold: there are none) */
    uint32_t w, h;          /* the image                                                                                       */
    uint32_t row0, rows;    /* the run of rows                                                                                 */
    uint32_t dtype;         /* decode_png.h DEBIG_PNG_L_*: uint8, uint16, int32, int64                                         */
    uint32_t sites;         /* decode_png.h DEBIG_PNG_DISTANCE_DIFFERS 0, _TO_VALUE 1                                          */
} debig_png_label_distance_rows_task;
typedef struct debig_png_label_distance_cols_task {
    uint64_t g_off;         /* the image's first g element, in bytes rel. to d_g                                               */
    uint64_t out_off;       /* the image's first output element, in bytes rel. to d_out                                        */
    uint32_t w, h;          /* the image                                                                                       */
    uint32_t x0, cols;      /* the strip                                                                                       */
    uint32_t cap;           /* 0: none, else 1 .. 32767: the result is min(D2, cap^2)                                          */
    uint32_t format;        /* decode_png.h DEBIG_PNG_DISTANCE_SQUARED 0 (int32), _ROOT 1 (float32)                            */
} debig_png_label_distance_cols_task;
int debig_hip_png_label_distance_rows_batch(const void *d_labels, void *d_g, const debig_png_label_distance_rows_task *d_tasks,
                                            uint32_t n_tasks, void *hip_stream);
int debig_hip_png_label_distance_cols_batch(const void *d_g, void *d_out, const debig_png_label_distance_cols_task *d_tasks, uint32_t n_tasks,
                                            void *hip_stream);

/* ---- connected components of a dense label tensor (csrc/png_label_components_kernel.inc, behind debig_png_label_components in
 * decode_png.h, which has the rule): union-find over the PARENT PLANE d_parent, one uint32 per element of the image (w x h, dense):
 * the index y * w + x of an element of the same component that is not larger than the element's own (a ROOT holds its own), or
 * 0xffffffff for a background element.  Five launches on one stream share one TASK, a run of whole rows of one image for one
 * workgroup of 256 lanes: rows x w <= DEBIG_PNG_LABEL_COMPONENTS_ELEMS, or one row.
 *   ROWS    reads the labels and writes every slot of its rows: the start of the element's horizontal run of equal values.
 *   MERGE   reads the labels of its rows and of the row above its first one, and joins the trees of neighbours in rows y - 1 and y
 *           for every row y > 0 of the task, WITH ATOMICS ON SLOTS ANYWHERE IN THE IMAGE'S PLANE.  It is the one launch whose
 *           workgroups write one structure together; afterwards the roots are the components' smallest elements, whatever the order.
 *           The plane after it is not a pure function of the input, what the next three make of it is.
 *   COUNT   d_counts[count_idx] = the roots in the task's rows.  The plane is only read from here on.
 *   NUMBER  (ids CONSECUTIVE only) every root of the task gets out = 1 + its rank in raster order among the image's roots: the sum
 *           of d_counts[count_first .. count_idx) plus its rank in the task.  The task sums those counts itself.
 *   FINISH  ids FIRST: out = the root above the element, background -1.  CONSECUTIVE: a non-root gets the out of its root,
 *           background 0; roots are left as NUMBER wrote them.
 * d_out is int32, 4 bytes per element.  The work of MERGE and FINISH depends on the data and on the race (the depth of the trees).
 * Every value read from the plane is checked before it is an index: one that is not below w x h, or above the slot it came from,
 * makes the slot a root.  No launch waits for another workgroup.  d_parent and d_counts must not overlap d_labels, d_out or each
 * other.  A task is skipped by every launch when dtype is above 3, connectivity is neither 4 nor 8, use_background or ids is above 1,
 * w or h is 0 or above 16384, rows is 0 or the run leaves the image, rows x w exceeds the cap with rows above 1, count_first is above
 * count_idx or more than 16383 below it, or an offset or address is not a multiple of the element size (of 4 for the plane, the
 * output and the counts). */
#define DEBIG_PNG_LABEL_COMPONENTS_ELEMS 16384u
typedef struct debig_png_label_components_task {
    uint64_t label_off;     /* the image's first element, in bytes rel. to d_labels                                            */
    uint64_t parent_off;    /* the image's first slot, in bytes rel. to d_parent                                               */
    uint64_t out_off;       /* the image's first output element, in bytes rel. to d_out                                        */
    int64_t background;     /* use_background 1: the elements equal to it belong to no component (a value the dtype cannot hold: none) */
    uint32_t w, h;          /* the image                                                                                       */
    uint32_t row0, rows;    /* the run of rows                                                                                 */
    uint32_t dtype;         /* decode_png.h DEBIG_PNG_L_*: uint8, uint16, int32, int64                                         */
    uint32_t connectivity;  /* 4: edge neighbours, 8: edge and corner neighbours                                               */
    uint32_t use_background;/* 0, 1                                                                                            */
    uint32_t ids;           /* decode_png.h DEBIG_PNG_COMPONENTS_FIRST 0, _CONSECUTIVE 1                                       */
    uint32_t count_idx;     /* the task's word in d_counts                                                                     */
    uint32_t count_first;   /* the word of the image's first task: the image's tasks have consecutive words, in row order      */
    uint32_t reserved[2];
} debig_png_label_components_task;
int debig_hip_png_label_components_rows_batch(const void *d_labels, void *d_parent, const debig_png_label_components_task *d_tasks,
                                              uint32_t n_tasks, void *hip_stream);
int debig_hip_png_label_components_merge_batch(const void *d_labels, void *d_parent, const debig_png_label_components_task *d_tasks,
                                               uint32_t n_tasks, void *hip_stream);
int debig_hip_png_label_components_count_batch(const void *d_parent, void *d_counts, const debig_png_label_components_task *d_tasks,
                                               uint32_t n_tasks, void *hip_stream);
int debig_hip_png_label_components_number_batch(const void *d_parent, const void *d_counts, void *d_out,
                                                const debig_png_label_components_task *d_tasks, uint32_t n_tasks, void *hip_stream);
int debig_hip_png_label_components_finish_batch(const void *d_parent, void *d_out, const debig_png_label_components_task *d_tasks,
                                                uint32_t n_tasks, void *hip_stream);

/* ---- PNG encode (csrc/png_encode_kernel.inc, behind debig_png_encode_batch in decode_png.h, which has the file's rules): two
 * launches on one stream.
 *   FILTER   a task is a run of rows of one image (rows x row_bytes <= DEBIG_PNG_ENCODE_FILTER_BYTES, or one row) for one workgroup
 *            of 256 lanes: it reads the dense tensor (HWC or CHW, elements of 1 / 2 / 4 / 8 bytes) and writes 1 + row_bytes bytes
 *            per row, the filter type and the filtered bytes, at stream_off + y * (1 + row_bytes); 16-bit samples big-endian.
 *            filter 0 .. 4: that type for every row; 5 (ADAPTIVE): per row the type with the smallest sum of min(b, 256 - b) over
 *            its filtered bytes, ties to the lowest type.  An element above 2^depth - 1 (int32 / int64: negative ones too), or not
 *            below palette_entries when that is not 0, stores 1 into d_flags[flag_idx]; the caller clears the flags.
 *   DEFLATE  a task is one chunk of an image's filtered stream, at most DEBIG_PNG_ENCODE_CHUNK bytes, for one wavefront.  It writes
 *            complete DEFLATE blocks that hold exactly the chunk's bytes into its slot, from the slot's first byte, and their byte
 *            count into d_counts[count_idx].  last 0: the output ends on a byte boundary with an empty stored block (00 00 FF FF)
 *            and sets no BFINAL; last 1: the last block has BFINAL, the bits up to the byte boundary are 0.  level 0: one stored
 *            block.  level 1: one fixed-Huffman block, greedy, matches of 3 .. 258 bytes at distances 1 .. 32768 that may start in
 *            the 32768 stream bytes in front of the chunk (never in front of the stream, never reading at or behind the chunk's
 *            end); if that is not smaller than the chunk stored, the chunk is written stored (flags & DEBIG_PNG_ENCODE_NO_STORED:
 *            never; tests).  The bytes are a pure function of the task and the stream: the same for every grid, order and run.
 *            NOT BUILT: dynamic Huffman blocks, lazy matching, levels above 1.
 * A filter task is skipped when dtype is above 3, channels is outside 1 .. 4, depth is neither 8 nor 16 or does not go with the dtype
 * (uint8: 8, uint16: 16), channels is above 1 with int32 / int64, layout is above 1, filter is above 5, palette_entries is above 256
 * or set with channels != 1 or depth != 8, w or h is 0 or above 16384, the run leaves the image or exceeds the budget with rows
 * above 1, or the image is not aligned to its element.  A deflate task is skipped when level or last is above 1, bpp is outside
 * 1 .. 8, chunk_len is 0 or above the chunk size, the chunk leaves the stream, stream_len does not fit 32 bits, slot_cap is below
 * DEBIG_PNG_ENCODE_SLOT(chunk_len), or the slot is not aligned to 4. */
#define DEBIG_PNG_ENCODE_CHUNK 32768u
#define DEBIG_PNG_ENCODE_FILTER_BYTES 65536u
#define DEBIG_PNG_ENCODE_SLOT(len) ((((uint64_t)(len) + (uint64_t)(len) / 8u + 32u) + 15u) & ~(uint64_t)15u) /* worst case of a chunk */
#define DEBIG_PNG_ENCODE_NO_STORED 1u
typedef struct debig_png_encode_filter_task {
    uint64_t image_off;       /* the image's first element, in bytes rel. to d_images                                           */
    uint64_t stream_off;      /* the image's filtered stream, in bytes rel. to d_streams                                        */
    uint32_t w, h;            /* the image                                                                                      */
    uint32_t row0, rows;      /* the run of rows                                                                                */
    uint32_t channels;        /* 1 .. 4                                                                                         */
    uint32_t dtype;           /* decode_png.h DEBIG_PNG_L_*: uint8, uint16, int32, int64                                        */
    uint32_t depth;           /* 8, 16                                                                                          */
    uint32_t layout;          /* decode_png.h DEBIG_PNG_LAYOUT_HWC 0, _CHW 1                                                    */
    uint32_t filter;          /* 0 .. 4, or 5: adaptive                                                                         */
    uint32_t palette_entries; /* 0: none                                                                                        */
    uint32_t flag_idx;        /* the image's word in d_flags                                                                    */
    uint32_t reserved;
} debig_png_encode_filter_task;
typedef struct debig_png_encode_deflate_task {
    uint64_t stream_off;      /* the image's filtered stream, in bytes rel. to d_streams                                        */
    uint64_t stream_len;      /* its length                                                                                     */
    uint64_t chunk_off;       /* the chunk's first byte, rel. to the stream                                                     */
    uint64_t slot_off;        /* the task's output, in bytes rel. to d_slots (a multiple of 4)                                  */
    uint32_t chunk_len;       /* 1 .. DEBIG_PNG_ENCODE_CHUNK                                                                    */
    uint32_t slot_cap;        /* at least DEBIG_PNG_ENCODE_SLOT(chunk_len)                                                      */
    uint32_t level;           /* 0, 1                                                                                           */
    uint32_t bpp;             /* channels x depth / 8: a distance that is always tried                                          */
    uint32_t last;            /* 1: the image's last chunk                                                                      */
    uint32_t count_idx;       /* the task's word in d_counts                                                                    */
    uint32_t flags;           /* DEBIG_PNG_ENCODE_NO_STORED                                                                     */
    uint32_t reserved;
} debig_png_encode_deflate_task;
int debig_hip_png_encode_filter_batch(const void *d_images, void *d_streams, const debig_png_encode_filter_task *d_tasks, void *d_flags,
                                      uint32_t n_tasks, void *hip_stream);
int debig_hip_png_encode_deflate_batch(const void *d_streams, void *d_slots, const debig_png_encode_deflate_task *d_tasks, void *d_counts,
                                       uint32_t n_tasks, void *hip_stream);

/* ---- PNG encode, level 2 (csrc/png_encode_dynamic_kernel.inc, behind debig_png_encode_batch_dyn in decode_png.h): the DEFLATE task
 * of above with one dynamic-Huffman block per chunk where that is smaller.
 *   DYNAMIC  a task is a deflate task (level 2) plus a token row: token_cap bytes at d_tokens + token_off (a multiple of 4), at
 *            least 4 x chunk_len, the task's own.  One wavefront runs level 1's matcher -- the SAME token sequence --, stores one
 *            32-bit token per literal or match into the row and counts the literal/length and distance symbols; builds the two
 *            codes and the code-length code by the rule below; knows the exact sizes of the chunk stored, in the fixed code and in
 *            the dynamic code (header included) before it writes; and writes the dynamic block iff dynamic_bits < fixed_bits and
 *            its bytes with the trailer are below the stored bytes (flags & DEBIG_PNG_ENCODE_NO_STORED waives the second
 *            condition), else exactly the bytes of level 1 for that task and those flags.  flags & DEBIG_PNG_ENCODE_ONLY_DYNAMIC
 *            (tests): the dynamic block whenever its bytes fit slot_cap, whatever the sizes say.  Slot, count, trailer, `last` and
 *            the purity of the bytes are those of the deflate task; per chunk level 2 <= level 1 <= level 0.
 *   The rule for an alphabet of n symbols with counts c[s] and limit L (15: literal/length, n 286, and distance, n 30; 7: the
 *   code-length code, n 19): the used symbols are those with c > 0; with fewer than two of them every used symbol gets length 1 and
 *   then the unused symbols of lowest index get length 1 until two symbols have it.  Else the used symbols are ordered by (count,
 *   index) ascending and a Huffman tree is built with two queues (leaves in that order, internal nodes in creation order; each step
 *   takes the two smallest weights, a leaf before an internal node of the same weight); num[l] counts the leaves of depth l, depths
 *   above L at L; while the Kraft total sum(num[l] << (L - l)) exceeds 1 << L: num[L] -= 1, the largest l < L with num[l] > 0 gives
 *   num[l] -= 1 and num[l + 1] += 2, total -= 1; the lengths are handed out along the order, the first num[L] symbols get L, the
 *   next num[L - 1] get L - 1, and so on; the codes are canonical (RFC 1951 3.2.2).  The header: HLIT = max(257, 1 + the last used
 *   literal/length symbol), HDIST = 1 + the last used distance symbol; the two length lists are one list, coded greedily from the
 *   front over maximal runs of one value v (v = 0: symbol 18 for min(run, 138) while run >= 11, then symbol 17 for a rest of
 *   3 .. 10, a rest of 1 .. 2 as zeros; v != 0: v once, symbol 16 for min(rest, 6) while rest >= 3, a rest of 1 .. 2 as v); HCLEN
 *   drops the trailing zeros of the RFC's order, down to 4.
 *   CODES    a task is (n counts of 32 bits at d_counts + counts_off, the limit) -> n length bytes at d_lens + lens_off, one
 *            wavefront per task, by the SAME device function: how tests reach the builder with histograms no stream produces.
 * A dynamic task is skipped when a deflate task with its fields would be (level: anything but 2), token_off is no multiple of 4 or
 * token_cap is below 4 x chunk_len.  A codes task is skipped when n is 0 or above 286, limit is 0 or above 15 or 1 << limit is
 * below n, counts_off is no multiple of 4, or a count is above DEBIG_PNG_ENCODE_CODES_MAX_COUNT (the weights are summed in 32 bits). */
#define DEBIG_PNG_ENCODE_ONLY_DYNAMIC 2u
#define DEBIG_PNG_ENCODE_ROUND_TASKS 2048u /* the host launches level 2 in rounds of so many tasks: 256 MiB of token rows */
#define DEBIG_PNG_ENCODE_CODES_MAX_COUNT (1u << 22)
typedef struct debig_png_encode_dynamic_task {
    uint64_t stream_off;      /* the fields of debig_png_encode_deflate_task ...                                                */
    uint64_t stream_len;
    uint64_t chunk_off;
    uint64_t slot_off;
    uint32_t chunk_len;
    uint32_t slot_cap;
    uint32_t level;           /* 2                                                                                              */
    uint32_t bpp;
    uint32_t last;
    uint32_t count_idx;
    uint32_t flags;           /* DEBIG_PNG_ENCODE_NO_STORED, DEBIG_PNG_ENCODE_ONLY_DYNAMIC                                      */
    uint32_t reserved;
    uint64_t token_off;       /* ... and the task's token row, in bytes rel. to d_tokens (a multiple of 4)                      */
    uint32_t token_cap;       /* its bytes, at least 4 x chunk_len                                                              */
    uint32_t reserved2;
} debig_png_encode_dynamic_task;
typedef struct debig_png_encode_codes_task {
    uint64_t counts_off;      /* n counts of 32 bits, in bytes rel. to d_counts (a multiple of 4)                               */
    uint64_t lens_off;        /* n length bytes, rel. to d_lens                                                                 */
    uint32_t n;               /* 1 .. 286                                                                                       */
    uint32_t limit;           /* 1 .. 15, 1 << limit >= n                                                                       */
} debig_png_encode_codes_task;
int debig_hip_png_encode_dynamic_batch(const void *d_streams, void *d_slots, void *d_tokens, const debig_png_encode_dynamic_task *d_tasks,
                                       void *d_counts, uint32_t n_tasks, void *hip_stream);
int debig_hip_png_encode_codes_batch(const void *d_counts, void *d_lens, const debig_png_encode_codes_task *d_tasks, uint32_t n_tasks,
                                     void *hip_stream);

/* ---- PNG encode, level 3 (csrc/png_encode_lz_kernel.inc, behind debig_png_encode_batch_lz in decode_png.h): the dynamic task of
 * above with another matcher in front of the same back end -- the token row, the code rule, the three sizes, the choice with
 * DEBIG_PNG_ENCODE_NO_STORED and DEBIG_PNG_ENCODE_ONLY_DYNAMIC, the emit, the trailer and the stored block are level 2's code, run on
 * level 3's tokens.  Per chunk level 3 is never longer than stored, debig_png_encode_bound holds, and the bytes are a pure function
 * of the task and the stream: the same for every grid, order and run.  Level 3 is NOT guaranteed to be at most level 2: the tokens
 * differ, and neither matcher is run to check the other.  It is made for label maps, instance ids and other flat tensors; on
 * photographs it changes next to nothing.
 *   THE RULE.  Chunks, the window and the table are level 1's and are not touched: ped_hash, the 4096 entries, position + 1 inserted
 *   by atomicMax, ped_window, and every lane of a step reading before any lane inserts.
 *   A task carries row_stride S.  S is 0 for none.  Otherwise bpp < S and S + bpp <= 32768.  The host passes S = 1 + width x
 *   channels x depth / 8 when that holds, else 0.  The kernel treats S as a plain distance and does not need it to be a real row.
 *   For position p of the chunk, gp = c0 + p and maxl = min(258, len - p).  If maxl < 3 then L(p) = 0.  Otherwise the candidates are
 *   tried in this order: 1. distance 1; 2. bpp, if bpp > 1; 3. S; 4. S - bpp; 5. S + bpp; 6. the table's candidate, if it is in
 *   front of gp, within 32768, and not one of the distances before it.  A candidate needs gp >= d.  A distance equal to an earlier
 *   one is skipped.  The longest match wins, and ties go to the earlier candidate.  Then, as at level 1, a best below 3, or of 3
 *   farther than 4096 (PED_TOO_FAR), is 0.
 *   The walk is greedy and wave-uniform with steps of 64, as at level 1.  It adds one deferral.  At an uncovered position q, the
 *   token is a literal when all of these hold: 3 <= L(q) < 16; q % 64 != 63; q + 1 < len; L(q + 1) > L(q).  Otherwise the token is
 *   the match, or a literal.  The check applies again at q + 1.  16 is zlib's max_lazy at its default level; the rule fixes it, it
 *   is not measured.  The last position of a step never defers, because its neighbour's length is not known yet.
 *   Tokens go to the token row in level 2's 32-bit format.
 * An lz task is skipped when a dynamic task with its fields would be (level: anything but 3), or row_stride is neither 0 nor
 * bpp < row_stride <= 32768 - bpp.
 * NOT BUILT: hash chains, a second or wider table, candidates beyond S +- bpp, several blocks per chunk, levels above 3, optimal
 * parsing. */
typedef struct debig_png_encode_lz_task {
    uint64_t stream_off;      /* the fields of debig_png_encode_dynamic_task ...                                                */
    uint64_t stream_len;
    uint64_t chunk_off;
    uint64_t slot_off;
    uint32_t chunk_len;
    uint32_t slot_cap;
    uint32_t level;           /* 3                                                                                              */
    uint32_t bpp;
    uint32_t last;
    uint32_t count_idx;
    uint32_t flags;           /* DEBIG_PNG_ENCODE_NO_STORED, DEBIG_PNG_ENCODE_ONLY_DYNAMIC                                      */
    uint32_t reserved;
    uint64_t token_off;
    uint32_t token_cap;
    uint32_t row_stride;      /* ... and S: 0, or the distance of the byte above, bpp < S <= 32768 - bpp                        */
} debig_png_encode_lz_task;
int debig_hip_png_encode_lz_batch(const void *d_streams, void *d_slots, void *d_tokens, const debig_png_encode_lz_task *d_tasks,
                                  void *d_counts, uint32_t n_tasks, void *hip_stream);

/* A byte span of a device arena. */
typedef struct debig_span {
    uint64_t off;
    uint64_t len;
} debig_span;

/* CRC-32 (kind 0; PNG chunk / gzip convention) or Adler-32 (kind 1; zlib) of n spans, one
 * result word per span.  Replaces the per-byte update_crc loop the reference runs over every
 * PNG chunk (src/decode_png.c:313-333, :862-874) and provides what it never verifies (gzip
 * CRC32 trailer, zlib Adler-32: src/decode_gz.c:281-297, src/decode_png.c:393-395).
 * Device pointers, asynchronous on hip_stream. */
int debig_hip_checksum_batch(const void *d_arena, const debig_span *d_spans, uint32_t *d_out,
                             uint32_t n, uint32_t kind, void *hip_stream);

/* Copy n byte ranges between device arenas (any alignment): the IDAT concatenation of
 * decode_png (src/decode_png.c:1285-1291) done in HBM. */
typedef struct debig_copy {
    uint64_t src_off;
    uint64_t dst_off;
    uint64_t len;
} debig_copy;
int debig_hip_gather(const void *d_src_arena, void *d_dst_arena, const debig_copy *d_copies,
                     uint32_t n, void *hip_stream);

/* plain device-to-device helpers used by the host layer (no torch needed) */
int debig_hip_device_count(void);
int debig_hip_set_device(int dev);
int debig_hip_get_device(void); /* the calling thread's current device, -1 on error */
uint64_t debig_hip_mem_free(void); /* free device memory of the current device in bytes, 0 on error */
void *debig_hip_malloc(uint64_t bytes);
void debig_hip_free(void *p);
int debig_hip_memcpy_h2d(void *d, const void *h, uint64_t bytes, void *hip_stream);
int debig_hip_memcpy_d2h(void *h, const void *d, uint64_t bytes, void *hip_stream);
int debig_hip_memset(void *d, int v, uint64_t bytes, void *hip_stream);
int debig_hip_stream_sync(void *hip_stream);
/* page-locked host memory (staging arenas of the host-buffer batch calls) */
void *debig_hip_host_alloc(uint64_t bytes);
void debig_hip_host_free(void *p);
const char *debig_hip_error_string(int err);
/* kernel timing on the stream the kernels run on (hipEvent based) */
void *debig_hip_event_create(void);
int debig_hip_event_record(void *ev, void *hip_stream);
float debig_hip_event_elapsed_ms(void *start, void *stop); /* synchronises on stop */
int debig_hip_event_sync(void *ev);
void debig_hip_event_destroy(void *ev);

#ifdef __cplusplus
}
#endif
#endif
