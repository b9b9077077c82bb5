/*
 * tessphot_hip.h -- C ABI of libtessphot_hip.so: the MI355X (gfx950) native per-target
 * photometry engine for the tasoc/photometry hot path.
 *
 * The reference is pure Python and has no FFI of its own; each entry point below names the
 * reference code (file:line, relative to the reference repository root) whose work it
 * replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 * -----------
 *  - every function returns int: 0 = TP_OK, < 0 = error code; tp_last_error(ctx) returns a
 *    ctx-owned, NUL-terminated description of the last failure on that ctx.
 *  - bulk data pointers named d_* are DEVICE pointers (HBM) obtained from tp_malloc (or any
 *    hipMalloc in the same process); pointers named h_* are host pointers.
 *  - the caller allocates and owns every buffer; the library never frees caller memory and
 *    keeps no pointer past the call.
 *  - all work is enqueued on the ctx's own HIP stream, in call order.  Calls return when
 *    the work is enqueued; tp_sync() (or a d2h copy) waits for it.
 *  - per-target failure is reported through int32 status arrays holding the reference's
 *    STATUS integers (photometry/BasePhotometry.py:48-59): 0 UNKNOWN, 1 OK, 2 ERROR,
 *    3 WARNING, 4 ABORT, 5 SKIPPED, 6 STARTED.  No C++ exception crosses the ABI.
 *  - one ctx per host thread; calls on one ctx are not thread-safe.
 *
 * Cube layout
 * -----------
 *  A stamp cube is float32 [n_targets][height][width][t_pitch]: per target exactly the
 *  reference's (rows, cols, times) C-order cube with TIME as the fastest axis
 *  (photometry/BasePhotometry.py:732), t_pitch >= n_cad elements between the time series
 *  of consecutive pixels.  t_pitch % 4 == 0 and a 16-byte aligned base select the
 *  128-bit load path; anything else still works on the scalar path.
 */
#ifndef TESSPHOT_HIP_H
#define TESSPHOT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TP_OK               0
#define TP_ERR_INVALID     -1   /* bad argument */
#define TP_ERR_HIP         -2   /* HIP runtime error (text in tp_last_error) */
#define TP_ERR_NOMEM       -3
#define TP_ERR_COMM        -4   /* RCCL error */
#define TP_ERR_UNSUPPORTED -5

/* STATUS integers, photometry/BasePhotometry.py:48-59 */
#define TP_STATUS_UNKNOWN 0
#define TP_STATUS_OK      1
#define TP_STATUS_ERROR   2
#define TP_STATUS_WARNING 3
#define TP_STATUS_ABORT   4
#define TP_STATUS_SKIPPED 5
#define TP_STATUS_STARTED 6

typedef struct tp_ctx tp_ctx;

typedef struct tp_cube_desc {
	int32_t n_targets;
	int32_t n_cad;      /* T: number of cadences */
	int32_t height;     /* H: stamp rows */
	int32_t width;      /* W: stamp columns */
	int64_t t_pitch;    /* elements between consecutive pixels' time series (>= n_cad) */
} tp_cube_desc;

/* ---- context, memory, timing ------------------------------------------------------------ */
int tp_version(void);
int tp_device_count(int* n);
int tp_ctx_create(int device, tp_ctx** out);
/* An additional context (= one more HIP stream) on the same device; high_priority != 0 asks for the
 * device's greatest stream priority (used for the latency-bound K2P2 stage of the chunked pipeline). */
int tp_ctx_create_stream(int device, int high_priority, tp_ctx** out);
int tp_ctx_destroy(tp_ctx* ctx);
const char* tp_last_error(tp_ctx* ctx);      /* ctx may be NULL: last tp_ctx_create failure */
int tp_device_info(tp_ctx* ctx, char* name, int name_len, int32_t* n_cu, uint64_t* hbm_bytes);
/* Free and total device memory as the driver counts them (either pointer may be NULL).  Blocks in the allocation cache of a context
 * (see tp_malloc) count as used: the figure is a lower bound of what the next allocations can get. */
int tp_mem_info(tp_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);
/* NUMA node of the device's PCIe slot (-1: unknown), for binding the host threads that feed it (device.bind_host_to_device). */
int tp_device_numa_node(int device, int* node);

/* Device memory.  tp_free keeps a block for the next tp_malloc of its size class (blocks up to 32 GiB, 160 GiB per context;
 * hipMalloc / hipFree of multi-GB blocks cost milliseconds and synchronise the device); a recycled block is handed out only
 * after everything that was queued on the context's stream when it was freed has run, so it is idle for whichever stream writes
 * it next.  tp_cache_trim gives the cached blocks back to the driver; when an allocation fails the library does so itself, for
 * this context first and then for every other context of the device. */
int tp_malloc(tp_ctx* ctx, uint64_t nbytes, void** d_ptr);
int tp_free(tp_ctx* ctx, void* d_ptr);
int tp_cache_trim(tp_ctx* ctx);
int tp_memset(tp_ctx* ctx, void* d_ptr, int value, uint64_t nbytes);
int tp_memcpy_h2d(tp_ctx* ctx, void* d_dst, const void* h_src, uint64_t nbytes);
int tp_memcpy_d2h(tp_ctx* ctx, void* h_dst, const void* d_src, uint64_t nbytes);   /* waits */
int tp_memcpy_d2d(tp_ctx* ctx, void* d_dst, const void* d_src, uint64_t nbytes);
/* Copy n_rows time series of n_cad float32 between pitched layouts (host -> device): the host
 * cube of BasePhotometry._load_cube (BasePhotometry.py:720-751) has pitch n_cad. */
int tp_upload_cube(tp_ctx* ctx, float* d_dst, int64_t dst_pitch, const float* h_src, int64_t src_pitch,
	int64_t n_rows, int64_t n_cad);
/* Pinned (page-locked) host memory and copies that return as soon as they are enqueued on the ctx stream: with a
 * second context (= stream) for the transfers and tp_event_* ordering, the upload of the next chunk of stamp cubes
 * overlaps the photometry of the current one -- the regime of a plugin that receives host cubes from
 * BasePhotometry._load_cube (BasePhotometry.py:720-751).  h_src / h_dst must come from tp_host_alloc. */
int tp_host_alloc(tp_ctx* ctx, uint64_t nbytes, void** h_ptr);
int tp_host_free(tp_ctx* ctx, void* h_ptr);
int tp_upload_cube_async(tp_ctx* ctx, float* d_dst, int64_t dst_pitch, const float* h_src, int64_t src_pitch,
	int64_t n_rows, int64_t n_cad);
int tp_memcpy_d2h_async(tp_ctx* ctx, void* h_dst, const void* d_src, uint64_t nbytes);
int tp_sync(tp_ctx* ctx);

/* Cross-stream ordering: several contexts on one device each own a HIP stream; an event recorded on one
 * context's stream can be waited for by another's (hipStreamWaitEvent), so independent stages of the
 * pipeline (memory-bound A1 / A6, latency-bound K2P2) of different target chunks overlap on the GPU. */
int tp_event_create(tp_ctx* ctx, void** event);
int tp_event_destroy(tp_ctx* ctx, void* event);
int tp_event_record(tp_ctx* ctx, void* event);           /* on ctx's stream */
int tp_stream_wait_event(tp_ctx* ctx, void* event);      /* ctx's stream waits for the event */
int tp_event_sync(tp_ctx* ctx, void* event);             /* the HOST waits for the event (reuse of a pinned staging buffer) */

/* HIP-event stopwatch on the ctx stream; slot in [0, 16). */
int tp_timer_start(tp_ctx* ctx, int slot);
int tp_timer_stop(tp_ctx* ctx, int slot);
int tp_timer_elapsed_ms(tp_ctx* ctx, int slot, float* ms);   /* waits for the stop event */

/* Per-kernel profile: when enabled every kernel launch is bracketed by HIP events on the
 * ctx stream.  kernel ids are dense in [0, tp_kernel_count()). */
int tp_profile_enable(tp_ctx* ctx, int on);
int tp_profile_reset(tp_ctx* ctx);
int tp_kernel_count(void);
const char* tp_kernel_name(int kernel_id);
int tp_profile_get(tp_ctx* ctx, int kernel_id, int64_t* n_launches, double* total_ms);   /* waits */

/* ---- A1: sum image ------------------------------------------------------------------------
 * replaces BasePhotometry.sumimage (photometry/BasePhotometry.py:1008-1019) and the FFI
 * accumulation of prepare.py:450-453,459: per-pixel mean over the cadences with
 * (quality & bitmask) == 0 (TESSQualityFlags.DEFAULT_BITMASK = 4335, quality.py:123-124),
 * non-finite pixels excluded from sum and count, zero count -> NaN.  float64 accumulation.
 *   d_quality: int32 [n_cad] shared by all targets (quality_target_stride = 0) or
 *              [n_targets][quality_target_stride].
 *   d_subtract: optional float32 [n_targets][subtract_pitch]: a stamp-constant background series
 *              subtracted on the fly (images := raw - background, prepare.py:419-420), or NULL.
 *   d_sumimage: float64 [n_targets][height*width].                                          */
int tp_sumimage(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images,
	const int32_t* d_quality, int64_t quality_target_stride, uint32_t bitmask,
	const float* d_subtract, int64_t subtract_pitch, double* d_sumimage);

/* ---- A2..A5b + A7: K2P2 aperture masks -------------------------------------------------------
 * replaces k2p2.k2p2FixFromSum (photometry/AperturePhotometry/k2p2v2.py:344-623: KDE-mode/MAD
 * threshold, DBSCAN clustering, watershed segmentation, size filter, hole filling, overflow
 * columns) and the mask selection, minimum aperture, edge test and contamination of
 * AperturePhotometry.do_photometry (photometry/AperturePhotometry/photometry.py:31-41, 93-131,
 * 220-254), for every target of the batch.  Stamps are fixed-size cubes: resize_stamp() cannot
 * grow them (BasePhotometry.py:605-612 -> False), so edge-touching masks are used as they are
 * and reported through the edge bits of d_flags for a host-side retry on a bigger cut-out.
 * Stamps of any size up to 32 767 pixels (labels and pixel indices are signed 16-bit): up to about 54 x 54 the work arrays are in LDS, beyond that in a context-owned
 * HBM scratch (same code, same results, slow: the few bright stars of a CCD).
 *   catalog (ragged, CSR): d_cat_offsets int64 [n_targets+1]; per star float32 column_stamp,
 *     row_stamp, tmag, column, row (BasePhotometry.catalog, BasePhotometry.py:1153-1178), int64 starid.
 *   d_target_pos_row/column: float64 CCD position (target_pos_row/column); d_target_tmag float64.
 *   d_aperture: int32 [n_targets][H*W] pixel flags (BasePhotometry.aperture; bit 1 = collected).
 *   d_cut_override: optional float64 [n_targets] replacing the KDE/Powell threshold CUT.
 *   params: NULL = the plugin's settings (photometry.py:54-64).
 * outputs: d_mask uint8 [n_targets][H*W] (final_phot_mask); d_status int32 STATUS;
 *   d_flags int32: bit0 minimum aperture used, bits1-4 mask touches stamp edge (row 0, last row,
 *   column 0, last column), bit5 K2P2NoStars, bit6 no mask passed the size filter,
 *   bits 8+ error kind (1 no flux, 2 zero KDE bandwidth, 3 no watershed peak, 4 target outside
 *   stamp, 5 too many masks, 6 no catalog star in mask, 7 empty KDE sample: every positive flux >= 70000);
 *   d_contamination float64 (AP_CONT, NaN if undefined); d_diag optional float64 [n_targets][8] =
 *   (CUT, MODE, MAD1, KDE bandwidth, FFT-grid mode guess, n positive pixels, min|S-CUT|, n masks);
 *   d_cat_in_mask optional uint8 [n_catalog]: star falls inside the final mask (skip_targets).   */
typedef struct tp_k2p2_params {
	double thresh;                  /* 0.8 */
	int32_t min_no_pixels_in_mask;  /* 4 */
	int32_t min_for_cluster;        /* 4 */
	int32_t extend_overflow;        /* 1 */
	int32_t reserved;
	double ws_thres;                /* 0 */
	double saturation_limit;        /* 7.0 */
} tp_k2p2_params;
int tp_k2p2_masks(tp_ctx* ctx, int32_t n_targets, int32_t height, int32_t width,
	const double* d_sumimage,
	const int64_t* d_cat_offsets, const float* d_cat_column_stamp, const float* d_cat_row_stamp, const float* d_cat_tmag,
	const float* d_cat_column, const float* d_cat_row, const int64_t* d_cat_starid,
	const double* d_target_pos_row, const double* d_target_pos_column, const double* d_target_tmag, const int64_t* d_target_starid,
	const int32_t* d_stamps, const int32_t* d_aperture, const double* d_cut_override, const tp_k2p2_params* params,
	uint8_t* d_mask, int32_t* d_status, int32_t* d_flags, double* d_contamination, double* d_diag, uint8_t* d_cat_in_mask);

/* ---- A6: aperture extraction ---------------------------------------------------------------
 * replaces the per-cadence loop of AperturePhotometry.do_photometry
 * (photometry/AperturePhotometry/photometry.py:172-201): in-mask flux (float32 np.sum order,
 * bit-exact), flux error sqrt(sum err^2), flux-weighted centroid over pixels with flux > 0 in
 * 1-based CCD (column, row) coordinates, np.nansum of the background (NaN -> 0, float32 np.sum order,
 * bit-exact); NaN rules of :182-201.
 *   d_backgrounds: bkg_mode 0: cube with the layout of desc;
 *                  bkg_mode 1: one series per target, float32 [n_targets][bkg_series_pitch]
 *                  (a stamp-constant background: every pixel of a cadence has the same value);
 *                  NULL: aperture-only (no background input): d_flux_background may be NULL too, and is
 *                  filled with NaN otherwise.
 *   d_subtract: optional float32 [n_targets][subtract_pitch] subtracted from d_images on the fly
 *                  (d_images then holds the raw, not background-subtracted, flux), or NULL.
 *   d_mask:   uint8 [n_targets][height*width], non-zero = in aperture (final_phot_mask).
 *   d_stamps: int32 [n_targets][4] = (row_min, row_max, col_min, col_max), BasePhotometry.stamp.
 *   d_status: optional int32 [n_targets]; targets whose status is TP_STATUS_ERROR are skipped
 *             (outputs untouched), like the early returns of photometry.py:116,163,170.
 *   outputs:  float64 [n_targets][out_pitch] each (lightcurve columns, BasePhotometry.py:425-428);
 *             d_centroid_col / d_centroid_row are pos_centroid[:,0] / [:,1].                   */
int tp_aperture_extract(tp_ctx* ctx, const tp_cube_desc* desc,
	const float* d_images, const float* d_images_err, const float* d_backgrounds,
	int32_t bkg_mode, int64_t bkg_series_pitch, const float* d_subtract, int64_t subtract_pitch,
	const uint8_t* d_mask, const int32_t* d_stamps, const int32_t* d_status,
	double* d_flux, double* d_flux_err, double* d_flux_background,
	double* d_centroid_col, double* d_centroid_row, int64_t out_pitch);

/* ---- A1 + A2..A5b + A7 + A6 fused: AperturePhotometry.do_photometry for a batch -------------------
 * replaces one pass of photometry/AperturePhotometry/photometry.py:75-257 over a fixed stamp for every
 * target: sum image, K2P2 mask (+ minimum aperture, contamination), extraction.  One wavefront owns a
 * target from the first load to the last store, the sum image and the mask stay in LDS in between; the
 * outputs are bit-identical to tp_sumimage + tp_k2p2_masks + tp_aperture_extract called in turn
 * (argument meaning as documented there; d_sumimage is an OUTPUT here).                              */
int tp_aperture_photometry(tp_ctx* ctx, const tp_cube_desc* desc,
	const float* d_images, const float* d_images_err, const float* d_backgrounds, int32_t bkg_mode, int64_t bkg_series_pitch,
	const float* d_subtract, int64_t subtract_pitch,
	const int32_t* d_quality, int64_t quality_target_stride, uint32_t bitmask,
	const int64_t* d_cat_offsets, const float* d_cat_column_stamp, const float* d_cat_row_stamp, const float* d_cat_tmag,
	const float* d_cat_column, const float* d_cat_row, const int64_t* d_cat_starid,
	const double* d_target_pos_row, const double* d_target_pos_column, const double* d_target_tmag, const int64_t* d_target_starid,
	const int32_t* d_stamps, const int32_t* d_aperture, const tp_k2p2_params* params,
	double* d_sumimage, uint8_t* d_mask, int32_t* d_status, int32_t* d_flags, double* d_contamination, double* d_diag,
	uint8_t* d_cat_in_mask,
	double* d_flux, double* d_flux_err, double* d_flux_background, double* d_centroid_col, double* d_centroid_row, int64_t out_pitch);
/* The same from a sum image the caller already holds (d_sumimage is an INPUT: float64 [n_targets][height*width], e.g. from
 * tp_background_sumimage, which forms it while it streams the raw cube for the background): the kernel starts at the K2P2 mask
 * (k2p2v2.py:388-623) and reads only the in-mask pixel rows of the cubes.  d_quality / bitmask are not used (the sum image
 * carries them) and may be NULL / 0.  Everything else as above; outputs bit-identical to tp_k2p2_masks + tp_aperture_extract. */
int tp_aperture_photometry_from_sumimage(tp_ctx* ctx, const tp_cube_desc* desc,
	const float* d_images, const float* d_images_err, const float* d_backgrounds, int32_t bkg_mode, int64_t bkg_series_pitch,
	const float* d_subtract, int64_t subtract_pitch,
	const int32_t* d_quality, int64_t quality_target_stride, uint32_t bitmask,
	const int64_t* d_cat_offsets, const float* d_cat_column_stamp, const float* d_cat_row_stamp, const float* d_cat_tmag,
	const float* d_cat_column, const float* d_cat_row, const int64_t* d_cat_starid,
	const double* d_target_pos_row, const double* d_target_pos_column, const double* d_target_tmag, const int64_t* d_target_starid,
	const int32_t* d_stamps, const int32_t* d_aperture, const tp_k2p2_params* params,
	const double* d_sumimage, uint8_t* d_mask, int32_t* d_status, int32_t* d_flags, double* d_contamination, double* d_diag,
	uint8_t* d_cat_in_mask,
	double* d_flux, double* d_flux_err, double* d_flux_background, double* d_centroid_col, double* d_centroid_row, int64_t out_pitch);

/* ---- B*, B2, B3: background on stamps -----------------------------------------------------------
 * tp_background_stamp (B*): build-defined stamp analogue of backgrounds.fit_background
 *   (photometry/backgrounds.py:52-211, which needs 64x64 tiles of a full frame): per (target, cadence)
 *   mask non-finite / > flux_cutoff / < 0 pixels (backgrounds.py:89-94), SigmaClip(3 sigma, 5 iterations,
 *   median / std), SExtractor mode estimate; more than exclude_percentile % masked pixels -> NaN.
 *   d_raw: cube of raw (not background-subtracted) flux; d_bkg: float32 [n_targets][bkg_pitch].
 * tp_smooth_time (B2): prepare.py:317-335, out[k] = nanmean(in[max(k-w,0) : min(k+w+1,T)]),
 *   w = time_smooth/2 (time_smooth = 3 at 1800 s cadence, 9 at 600 s; prepare.py:258), float32.
 * tp_subtract_background (B3): prepare.py:419-425, images = raw - bkg[k] (float32); pixels whose
 *   flag & flag_mask != 0 (PixelQualityFlags.ManualExclude = 2) become NaN in image and error.
 *   d_pixel_flags: optional uint8 [n_targets][H*W][n_cad]; d_raw_err / d_images_err optional;
 *   in-place (d_images == d_raw) is allowed; bkg_pitch >= t_pitch.                               */
int tp_background_stamp(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_raw,
	double flux_cutoff, double exclude_percentile, float* d_bkg, int64_t bkg_pitch);
int tp_smooth_time(tp_ctx* ctx, int32_t n_targets, int32_t n_cad, int64_t pitch, int32_t time_smooth,
	const float* d_in, float* d_out);
int tp_subtract_background(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_raw, const float* d_raw_err,
	const float* d_bkg, int64_t bkg_pitch, const uint8_t* d_pixel_flags, uint32_t flag_mask,
	float* d_images, float* d_images_err);
/* B* + B2 + A1 in ONE pass over the raw cube: d_bkg_raw = tp_background_stamp(d_raw), d_bkg = tp_smooth_time(d_bkg_raw)
 * (prepare.py:258, 317-335), d_sumimage = tp_sumimage(d_raw, d_subtract = d_bkg), i.e. the good-cadence mean of
 * float32(raw - smoothed background) per pixel (prepare.py:419-421, 450-459; BasePhotometry.py:1008-1019).  Both series
 * float32 [n_targets][bkg_pitch] and bit-identical to the two stand-alone entries; the sum image float64
 * [n_targets][height*width], equal to tp_sumimage's to rounding (another order of the float64 additions).  Stamps up to
 * 256 pixels and time_smooth <= 17 read the cube once; anything else runs the three entries in turn.                    */
int tp_background_sumimage(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_raw,
	double flux_cutoff, double exclude_percentile, int32_t time_smooth,
	const int32_t* d_quality, int64_t quality_target_stride, uint32_t bitmask,
	float* d_bkg_raw, float* d_bkg, int64_t bkg_pitch, double* d_sumimage);

/* ---- B1 + full-frame B2 / B3 / A1: the prepare stage on a frame stack ----------------------------------------
 * Frames: float32 [n_frames][frame_rows][row_pitch] resident in HBM (frame k at + k * frame_stride), as for tp_cut_stamps.
 * Layout of every pointer of this family (tests/test_gpu_frame_layouts.py holds each entry to it):
 *   - an entry that takes row_pitch and frame_stride addresses pixel (k, r, c) at k * frame_stride + r * row_pitch + c and requires
 *     row_pitch >= frame_cols and frame_stride >= frame_rows * row_pitch; an entry that takes n_pixels and frame_stride only reads
 *     contiguous images (pixel p of frame k at k * frame_stride + p, frame_stride >= n_pixels).  Elements between the rows, between
 *     the frames and after the last frame are never read and, in an output, never written.  The base pointer may point into a
 *     larger allocation (a window of a wider stack: row_pitch = the full width); no entry assumes an alignment of the base
 *     pointer, the pitch or the stride beyond that of a float (all loads and stores are single elements).
 *   - tp_background_mesh / _mesh_radial: d_frames with row_pitch / frame_stride.  d_exclude and d_subtract are DENSE
 *     [frame_rows][frame_cols] whatever row_pitch is, frame k at + k * exclude_frame_stride / subtract_frame_stride; each stride is
 *     0 (one image for all frames) or >= frame_rows * frame_cols, anything else is rejected.  d_mesh, d_nmasked dense [n_frames][ny][nx].
 *   - tp_background_zoom: d_background is written with row_pitch / frame_stride (the image pixels only); frame_stride below
 *     frame_rows * row_pitch is rejected, and so is a mesh that does not cover the frame (mesh_rows * box_size < frame_rows, or
 *     the same for the columns).  d_coef dense [n_frames][mesh_rows][mesh_cols], d_vmin / d_vmax [n_frames].
 *   - tp_frames_smooth_time: d_in and d_out have the SAME layout, frame k at + k * frame_stride in both; of d_out the n_pixels values
 *     of every frame are written, the frame_stride - n_pixels elements after them are not.
 *   - tp_frames_sumimage: d_images with frame_stride; d_quality [n_frames]; d_sumimage dense [n_pixels].
 *   - tp_frames_subtract: every pointer dense [n_values] (no pitch).
 * tp_background_mesh (B1, first half): the low-resolution mesh of backgrounds.fit_background for a plain image
 *   (photometry/backgrounds.py:89-97 pixel mask; :200-206 photutils Background2D on box_size x box_size cells with
 *   SigmaClip(3, maxiters = 5) and the SExtractor estimator): d_mesh float64 [n_frames][ny][nx] (NaN for a cell without an
 *   unmasked pixel), d_nmasked int32 [n_frames][ny][nx] (masked, padded or sigma-clipped pixels of the cell: photutils' mesh_nmasked, what its
 *   second mesh selection compares with exclude_percentile), ny = ceil(rows / box_size).
 *   d_exclude: optional uint8 manual-exclude image(s) [frame_rows][frame_cols] (exclude_frame_stride 0 = one for all frames).
 *   d_subtract: optional float32 image(s) [frame_rows][frame_cols] taken off the pixel values after the masking (the radial
 *   component of a TESS image, :200: Background2D(img0 - img_bkg_radial, mask = mask)).
 * tp_background_zoom (B1, second half): the full-resolution background from the cubic-spline coefficients of the finished
 *   mesh (after the exclusion of mostly-masked cells, their IDW fill, the 3 x 3 median filter and the spline prefilter --
 *   host work on ny x nx values per frame, photometry_amd/prepare.py), i.e. scipy.ndimage.zoom(order 3, mode 'reflect',
 *   grid_mode) as photutils' BkgZoomInterpolator calls it, clipped to [d_vmin[k], d_vmax[k]]; float32 output (what the
 *   reference's smoothing block stores, prepare.py:327).
 * tp_frames_smooth_time (B2, prepare.py:317-335), tp_frames_subtract (B3, prepare.py:419-425; flags uint8 per value) and
 *   tp_frames_sumimage (A1, prepare.py:450-453, 459) are the image-layout versions of tp_smooth_time,
 *   tp_subtract_background and tp_sumimage.                                                                          */
int tp_background_mesh(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols,
	int64_t row_pitch, int64_t frame_stride, const uint8_t* d_exclude, int64_t exclude_frame_stride,
	const float* d_subtract, int64_t subtract_frame_stride,
	double flux_cutoff, int32_t box_size, double* d_mesh, int32_t* d_nmasked);
/* tp_background_mesh_finish: the low-resolution part of photutils Background2D after the cell statistics, per frame on the device:
 *   cells with more than exclude_percentile % masked pixels (of box_size^2) or a non-finite statistic are replaced by the
 *   inverse-distance weighted mean of the 10 nearest kept cells, the filter_size x filter_size NaN-ignoring median filter, then
 *   d_vmin / d_vmax (range of the filtered mesh) and d_coef float64 [n_frames][rows][cols] = the cubic B-spline coefficients
 *   scipy.ndimage.zoom(order 3, mode 'reflect') interpolates from (spline_filter1d along both axes) -- the inputs of
 *   tp_background_zoom.  d_filtered optional: the filtered mesh itself.  A frame without a kept cell is NaN.  <= 8192 cells.  */
int tp_background_mesh_finish(tp_ctx* ctx, const double* d_mesh, const int32_t* d_nmasked, int32_t n_frames, int32_t mesh_rows,
	int32_t mesh_cols, int32_t box_size, double exclude_percentile, int32_t filter_size, double* d_coef, double* d_vmin, double* d_vmax,
	double* d_filtered);
int tp_background_zoom(tp_ctx* ctx, const double* d_coef, const double* d_vmin, const double* d_vmax, int32_t n_frames,
	int32_t mesh_rows, int32_t mesh_cols, int32_t box_size, int32_t frame_rows, int32_t frame_cols, int64_t row_pitch, int64_t frame_stride,
	float* d_background);
int tp_frames_smooth_time(tp_ctx* ctx, int32_t n_frames, int64_t n_pixels, int64_t frame_stride, int32_t time_smooth,
	const float* d_in, float* d_out);
int tp_frames_subtract(tp_ctx* ctx, int64_t n_values, const float* d_raw, const float* d_raw_err, const float* d_bkg,
	const uint8_t* d_pixel_flags, uint32_t flag_mask, float* d_images, float* d_images_err);
int tp_frames_sumimage(tp_ctx* ctx, int32_t n_frames, int64_t n_pixels, int64_t frame_stride, const float* d_images,
	const int32_t* d_quality, uint32_t bitmask, double* d_sumimage);

/* ---- pixel flags: "background shenanigans"  -------------------------------------------------
 * tp_frames_median_filter replaces pixel_flags.pixel_background_shenanigans (photometry/pixel_flags.py:61-79):
 *   scipy.ndimage.median_filter(img - SumImage, size) with the default 'reflect' boundary, for every frame of a stack;
 *   d_reference: float64 [frame_rows][frame_cols] (the sum image) or NULL; size odd, <= 15 (the reference uses 15);
 *   float32 output (what prepare.py:533-537 stores); non-finite input values sort to the end of a window.
 *   Layout: d_frames with row_pitch / frame_stride; d_reference DENSE [frame_rows][frame_cols], shared by all frames; d_out has
 *   the layout of d_frames -- output pixel (k, r, c) at k * frame_stride + r * row_pitch + c, NOT a dense [n_frames][rows][cols]
 *   buffer: it must be as large as the input stack; the padding between its rows and frames is not written.  Every size runs one
 *   of three kernels (15 on frames of at least 15 x 15; 9, 11, 13 on frames at least as large as the window; everything else).
 * tp_frames_block_median_accumulate: one block of the "mean shenanigans" (prepare.py:558-575): acc += nanmedian over the
 *   n_block <= 32 frames listed in d_frame_index (per pixel, NaN result -> 0); the caller divides by the number of blocks.
 *   d_frames: contiguous images, frame k at + k * frame_stride (>= n_pixels); d_frame_index int32 [n_block], every entry a frame
 *   of the stack (not checked); d_accumulator dense float64 [n_pixels].
 * tp_frames_threshold_flags: prepare.py:594-607: clears flag_bit in every pixel flag and sets it where
 *   |indicator - mean| > threshold (PixelQualityFlags.BackgroundShenanigans, bkgshe_threshold = 40).              */
/* tp_frames_pixel_flags: the per-frame pixel flags of the prepare stage (prepare.py:296-297, 406-408): bit_background
 *   (PixelQualityFlags.NotUsedForBackground) where fit_background masks the pixel (backgrounds.py:89-97: not finite, above
 *   flux_cutoff, negative, manually excluded), bit_manual (ManualExclude) where pixel_flags.pixel_manual_exclude (:13-58) does:
 *   columns >= d_first_excluded_column[k] (the host evaluates the header rules; NULL = no rule fires), and the whole frame when
 *   every pixel of it is zero and zero_is_excluded (TESS data).  d_all_zero int32 [n_frames] (out): the zero test per frame.
 *   d_pixel_flags uint8 [n_frames][rows][cols]; passed as d_exclude to tp_background_mesh / tp_radial_* it is exactly the mask.
 *   Layout: the zero test walks a frame as one run of rows * cols values, so the rows must be contiguous: row_pitch != frame_cols
 *   is rejected ("frames must be contiguous images") before anything is written; frame_stride may exceed rows * cols.  d_all_zero
 *   and d_pixel_flags are dense.
 * tp_frames_used_in_background: backgrounds_pixels_used (prepare.py:435, 464-466): d_used uint8 [n_pixels] = the pixel's
 *   bit_background is clear in more than threshold of the frames.                                                    */
int tp_frames_pixel_flags(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols,
	int64_t row_pitch, int64_t frame_stride, const int32_t* d_first_excluded_column, int32_t zero_is_excluded, double flux_cutoff,
	uint32_t bit_background, uint32_t bit_manual, int32_t* d_all_zero, uint8_t* d_pixel_flags);
int tp_frames_used_in_background(tp_ctx* ctx, const uint8_t* d_pixel_flags, int32_t n_frames, int64_t n_pixels, uint32_t bit_background,
	double threshold, uint8_t* d_used);
int tp_frames_median_filter(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols,
	int64_t row_pitch, int64_t frame_stride, const double* d_reference, int32_t size, float* d_out);
int tp_frames_block_median_accumulate(tp_ctx* ctx, const float* d_frames, int64_t n_pixels, int64_t frame_stride,
	const int32_t* d_frame_index, int32_t n_block, double* d_accumulator);
int tp_frames_threshold_flags(tp_ctx* ctx, const float* d_indicator, const double* d_mean, double threshold, uint32_t flag_bit,
	int64_t n_pixels, int32_t n_frames, uint8_t* d_pixel_flags);

/* ---- B1, TESS branch: the radial component of fit_background (photometry/backgrounds.py:104-197) ---------------
 * Frames: float32 [n_frames][n_pixels] contiguous images (row_pitch == frame_cols), frame k at + k * frame_stride (>= n_pixels).
 * The images beside the frames -- d_square, d_exclude (tp_radial_zeropoint / _ring_modes and their _zoom forms) and d_add
 * (tp_radial_evaluate) -- are contiguous too, frame k at + k * square_frame_stride / exclude_frame_stride / add_frame_stride: each
 * stride is 0 (one image for all frames) or >= n_pixels, anything else is rejected; a stride that comes with a NULL pointer is
 * ignored.  d_out of tp_radial_evaluate(_zoom) is written with frame_stride (the n_pixels values of every frame only).  A
 * tp_zoom_image must cover the frame (mesh_rows * box_size >= rows, mesh_cols * box_size >= frame_cols) or is rejected.
 * d_ring_pixels holds pixel indices below n_pixels (not checked).  The
 * pixel mask (:89-97) is evaluated on d_frames; values are d_frames - d_square (float64) once a square (mesh) component of
 * a previous iteration exists, d_frames alone (float32 arithmetic, as numpy does it) when d_square is NULL.
 * tp_radial_zeropoint: d_zeropoint[k] = -min(values over the unmasked pixels) + 1.0 (:166-168); NaN when everything is
 *   masked.  d_partial: float64 scratch [n_frames][n_partial].
 * tp_radial_ring_modes: _reduce_mode (:20-32) of log10(values + zeropoint) over the pixels of every ring (the callable
 *   statistic of scipy.stats.binned_statistic, :171-176): d_ring_pixels int32 [n_ring_pixels] lists the pixels of ring 0,
 *   ring 1, ... (row-major inside a ring), ring j = d_ring_pixels[d_ring_offsets[j] .. d_ring_offsets[j + 1]).
 *   statsmodels KDEUnivariate(x).fit(gridsize = 2000): Gaussian kernel, FFT on 2048 grid points, cut = 3, bandwidth
 *   bandwidth_constant * min(std, IQR / 1.349) * n^(-1/5) (bw = 'normal_reference'); zero bandwidth -> median; the mode is
 *   support[argmax(density)].  d_modes float64 [n_frames][n_rings] (NaN: fewer than 2 pixels), d_counts optional int32
 *   [n_frames][n_rings], d_scratch float64 [n_frames][n_ring_pixels].
 * tp_radial_evaluate: d_out = float32(10**s(r) - zeropoint + d_add) with r = hypot(col + col_offset - xcen, row - ycen)
 *   and s the cubic spline of frame k in FITPACK form (knots d_knots[k][0..n), coefficients d_coefs[k][..], n =
 *   d_n_knots[k] <= max_knots; evaluated with ext = 3, :186-188); n == 0: no radial component (d_out = d_add or 0).
 *   d_add optional float32 images (the square component: the total background of :209).                            */
/* Images that are evaluated where they are read instead of stored (round 5: the alternation read and wrote each of them
 * several times per iteration -- 304 MB of traffic per 2048 x 2048 frame against 117 MB of algorithmic bytes):
 *   tp_zoom_image   the square component, i.e. what tp_background_zoom would write, from the outputs of
 *                   tp_background_mesh_finish (d_coef / d_vmin / d_vmax); frame_cols = columns of the frame;
 *   tp_radial_image the radial component, i.e. what tp_radial_evaluate would write without d_add, from the ring profile
 *                   (tp_radial_profiles) and the zero point.
 * The *_zoom / *_radial entries below take them in place of d_square / d_subtract / d_add and give bit-identical results. */
typedef struct tp_zoom_image {
	const double* d_coef; const double* d_vmin; const double* d_vmax;
	int32_t mesh_rows, mesh_cols, box_size, frame_cols;
} tp_zoom_image;
typedef struct tp_radial_image {
	double col_offset, xcen, ycen;
	const double* d_knots; const double* d_coefs; const int32_t* d_n_knots;
	const double* d_zeropoint;
	int32_t max_knots, reserved;
} tp_radial_image;
int tp_radial_zeropoint(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride,
	const float* d_square, int64_t square_frame_stride, const uint8_t* d_exclude, int64_t exclude_frame_stride, double flux_cutoff,
	double* d_partial, int32_t n_partial, double* d_zeropoint);
int tp_radial_ring_modes(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride,
	const float* d_square, int64_t square_frame_stride, const uint8_t* d_exclude, int64_t exclude_frame_stride, double flux_cutoff,
	const double* d_zeropoint, const int32_t* d_ring_pixels, const int32_t* d_ring_offsets, int32_t n_rings, int32_t n_ring_pixels,
	double bandwidth_constant, double* d_scratch, double* d_modes, int32_t* d_counts);
/* tp_radial_profiles: the ring profile of every frame on the device (backgrounds.py:178-187): utilities.move_median_central of the
 *   ring modes (width radial_smooth, 0 = none; NaN-ignoring, ends redone over the first / last k + 2 points) and the interpolating
 *   cubic spline through the rings that have a mode, in FITPACK form (interior knots on the data points x[2 .. m-3], the m x m
 *   collocation system solved in the band) -- what InterpolatedUnivariateSpline(k = 3) returns, to rounding.  d_modes float64
 *   [n_frames][n_rings] (tp_radial_ring_modes), d_bin_center float64 [n_rings]; outputs as tp_radial_evaluate takes them
 *   (d_knots / d_coefs float64 [n_frames][max_knots], d_n_knots int32; 0 = no radial component: fewer than 4 usable rings --
 *   the reference logs for fewer than 3 and FITPACK refuses exactly 3).  n_rings <= 64.                           */
int tp_radial_profiles(tp_ctx* ctx, int32_t n_frames, int32_t n_rings, const double* d_modes, const double* d_bin_center,
	int32_t radial_smooth, int32_t max_knots, double* d_knots, double* d_coefs, int32_t* d_n_knots);
int tp_radial_evaluate(tp_ctx* ctx, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int64_t frame_stride,
	double col_offset, double xcen, double ycen, const double* d_knots, const double* d_coefs, const int32_t* d_n_knots, int32_t max_knots,
	const double* d_zeropoint, const float* d_add, int64_t add_frame_stride, float* d_out);
int tp_radial_zeropoint_zoom(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride,
	const tp_zoom_image* square, const uint8_t* d_exclude, int64_t exclude_frame_stride, double flux_cutoff,
	double* d_partial, int32_t n_partial, double* d_zeropoint);
int tp_radial_ring_modes_zoom(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride,
	const tp_zoom_image* square, const uint8_t* d_exclude, int64_t exclude_frame_stride, double flux_cutoff,
	const double* d_zeropoint, const int32_t* d_ring_pixels, const int32_t* d_ring_offsets, int32_t n_rings, int32_t n_ring_pixels,
	double bandwidth_constant, double* d_scratch, double* d_modes, int32_t* d_counts);
/* d_out = float32(radial + square): the total background of backgrounds.py:209 from the two implicit images */
int tp_radial_evaluate_zoom(tp_ctx* ctx, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int64_t frame_stride,
	const tp_radial_image* radial, const tp_zoom_image* add, float* d_out);
/* tp_background_mesh with the radial component to subtract (backgrounds.py:200) evaluated from its ring profile; max_knots <= 72 */
int tp_background_mesh_radial(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols,
	int64_t row_pitch, int64_t frame_stride, const uint8_t* d_exclude, int64_t exclude_frame_stride,
	const tp_radial_image* radial, double flux_cutoff, int32_t box_size, double* d_mesh, int32_t* d_nmasked);

/* ---- P1..P4: linear PSF photometry ----------------------------------------------------------------
 * tp_linpsf_prf (P1) replaces the per-target PRF construction of PSF.__init__ (photometry/psf.py:
 *   101-119).  The interpolating-spline fit is linear in the data, so the coefficient table of the
 *   inverse-distance blend is the same blend of the per-sample tables (fitted once per camera/CCD on
 *   the host with the reference's own scipy call, see photometry_amd/psf.py):
 *     d_coef[t][c] = sum_s d_weights[t][s] * d_base_coef[s][c]
 *   d_base_coef float64 [n_samples][n_coef], d_weights float64 [n_targets][n_samples] (already divided
 *   by the normalisation of psf.py:116), d_coef float64 [n_targets][n_coef].  n_samples <= 32.
 * tp_linpsf_fit (P2-P4) replaces PSF.integrate_to_image (psf.py:122-148), lsfit and the loop / status
 *   logic of LinPSFPhotometry.do_photometry (photometry/linpsf_photometry.py:22-34, 79-219).
 *   d_coef: [n_targets][n*n] spline coefficients, first axis = column direction (psf.py:119,146);
 *   d_knots_x / d_knots_y: [n+4] FITPACK knots of ANY strictly increasing sample grid, n = 4 .. 2048 (both axes alike; different
 *   lengths: tp_linpsf_fit_xy);
 *   cutoff_radius: any positive radius, +infinity = none (psf.py:142 `cutoff_radius is None`).  The SPOC layout -- evenly
 *   spaced, 9 samples per pixel, n = 32 .. 140 -- with a radius whose pixel edges stay inside the evenly spaced knots
 *   (cutoff_radius <= 5.25; LinPSFPhotometry uses 5, linpsf_photometry.py:63) runs on the fast kernels below; the library reads
 *   that off the knots on the device, and everything else is fitted by general kernels that evaluate the FITPACK box integral
 *   of psf.py:146 (dblint / fpintb: limits cut to the grid, so pixels beyond the PRF's support contribute zero) per star,
 *   pixel and cadence, with run-time sized normal equations -- same results, ~100 x slower (tp_linpsf_last_counts [13]).
 *   fitted stars (ragged, CSR): d_star_offsets int64 [n_targets+1]; d_target_index int32 [n_targets]
 *   = index of the main target among its fitted stars (the selection of linpsf_photometry.py:93-104 is
 *   host catalogue work); d_pos_row / d_pos_col float64 [n_fit_stars][pos_pitch] = row_stamp /
 *   column_stamp of every fitted star at every cadence, i.e. what catalog_attime() returns
 *   (BasePhotometry.py:1224-1258: WCS / jitter interpolation on the host).  max_stars = the largest number of
 *   fitted stars of a target, <= 64 (up to 8 stars run out of registers; more -- rare, crowded fields -- out of an HBM
 *   scratch with the same arithmetic: the reference's star selection has no limit, linpsf_photometry.py:93-104).
 *   d_subtract: optional background series subtracted from d_images on the fly (as in tp_sumimage).
 *   outputs: d_flux / d_flux_err float64 [n_targets][out_pitch] (flux_err is NaN, :169);
 *   d_fluxes_all float64 [n_fit_stars][out_pitch] every fitted flux; d_contamination float64 (PSF_CONT,
 *   :203-211); d_status int32 (OK, WARNING if contamination > 0.1, ERROR if all fluxes are NaN);
 *   d_fluxes_mean optional float64 [n_fit_stars].
 * tp_linpsf_set_path chooses between the two mappings of the fit that exist for targets with up to 4 fitted stars, up to 256
 *   pixels within reach of their cut-off circles and stars that visit at most 3 x 3 knot intervals of the PRF grid: 1 (default)
 *   the matrix-core kernel (v_mfma_f64_16x16x4_f64 on ONE tensor-product quartic spline per star and pixel, cadences in
 *   their natural order, the target's coefficients resident in LDS); 0 the vector-ALU kernels (one cadence per lane, cadences
 *   sorted by table origin, scalar-loaded polynomial coefficients) for every target.  Targets that do not qualify take the
 *   vector-ALU kernels either way.  Same results to rounding (1e-13).   */
/* tp_linpsf_fit / tp_psf_fit for a PRF spline whose two axes have different numbers of samples (psf.py:119 accepts any
 * RectBivariateSpline): d_coef [n_targets][n_coef_axis_x * n_coef_axis_y] (first axis = column direction), d_knots_x
 * [n_coef_axis_x + 4], d_knots_y [n_coef_axis_y + 4]; such a table is never the SPOC layout and is fitted by the any-grid kernels
 * (the FITPACK box integral).  With equal axis lengths they ARE tp_linpsf_fit / tp_psf_fit. */
int tp_linpsf_fit_xy(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images,
	const float* d_subtract, int64_t subtract_pitch,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis_x, int32_t n_coef_axis_y, int32_t max_stars,
	const int64_t* d_star_offsets, const int32_t* d_target_index,
	const double* d_pos_row, const double* d_pos_col, int64_t pos_pitch, double cutoff_radius,
	double* d_flux, double* d_flux_err, double* d_fluxes_all, int64_t out_pitch,
	double* d_contamination, int32_t* d_status, double* d_fluxes_mean);
int tp_psf_fit_xy(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images, const float* d_backgrounds,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis_x, int32_t n_coef_axis_y,
	const int64_t* d_star_offsets, const double* d_params0, const uint8_t* d_mini_aperture,
	double variance_floor, double cutoff_radius, int32_t maxiter_first, int32_t maxiter,
	double* d_flux, double* d_flux_err, double* d_centroid_row, double* d_centroid_col, int64_t out_pitch,
	double* d_params_out, int32_t* d_nit, int32_t* d_status);
int tp_linpsf_prf(tp_ctx* ctx, int32_t n_targets, int32_t n_samples, int32_t n_coef,
	const double* d_base_coef, const double* d_weights, double* d_coef);
int tp_linpsf_set_path(tp_ctx* ctx, int32_t path);
/* Which kernels fitted the targets of the LAST tp_linpsf_fit call of this context (the plan kernel decides per target):
 * counts[0] targets on the matrix cores, [1] the segments their series were cut into (a star that drifts over more than three
 * knot intervals gets one spline per stretch of the series; without drift one segment per target), [2] targets on the
 * vector-ALU polynomial kernels, [3] on the general kernel (wide excursions inside 16 cadences), [4] with more than 8 fitted
 * stars, [5..8] matrix-core targets with 1..4 fitted stars, [9..12] their segments, [13] targets fitted by the any-grid / any-radius
 * kernels (then all of them, and [0..12] are zero).  n <= 16 counters are copied. */
int tp_linpsf_last_counts(tp_ctx* ctx, int64_t* counts, int32_t n);
/* The positions a fit takes, for a field that moves as a whole: d_pos[s][k] = (double)(d_base[s] + d_shift[k]) -- the float32 sum the
 * plugin's catalogue holds after catalog_attime (BasePhotometry.py:1224-1258) for a translation, widened as
 * linpsf_photometry.py:116-121 does -- for n_stars stars and n_cad cadences, pos_pitch >= n_cad doubles per star.  (Built on the
 * host these arrays were most of the batched LinPSF entry's time: 75 MB for 2 000 targets.) */
int tp_star_positions(tp_ctx* ctx, int64_t n_stars, int32_t n_cad, const float* d_base, const float* d_shift, double* d_pos, int64_t pos_pitch);
/* The same for stars of many targets that each move by a series of their own -- a group of target pixel files, POS_CORR1/2 being per
 * file: d_pos[s][k] = (double)(d_base[s] + (float)d_shift[t][j]) with t = d_star_target[s] and j = d_lookup[t][k], or j = k when
 * d_lookup is NULL.  d_base [n_stars] float32 (row_stamp or column_stamp); d_star_target [n_stars]; d_shift [n_targets][shift_pitch]
 * float64 as loaded (the sum is the plugin's `cat['row_stamp'] + np.float32(jit[k, 1])`, BasePhotometry.catalog_attime for a source
 * with `jitter`, widened as linpsf_photometry.py:116-121 does; a NaN shift gives a NaN position); d_lookup [n_targets][lookup_pitch]
 * cadence -> row of d_shift: the plugin's argmin(|tref - tref[k]|), which is k itself for a finite, strictly increasing tref.
 * pos_pitch >= n_cad, lookup_pitch >= n_cad, shift_pitch >= n_cad without a lookup and >= 1 with one; d_pos beyond n_cad in a row is
 * left as it is.  A star whose target is outside [0, n_targets) and a lookup outside [0, shift_pitch) are not followed: the position
 * is NaN.  All offsets are 64-bit (4 096 files x a few stars x 19 008 doubles pass 2^31 bytes). */
int tp_star_positions_targets(tp_ctx* ctx, int64_t n_stars, int32_t n_cad, const float* d_base, const int32_t* d_star_target,
	const double* d_shift, int64_t shift_pitch, const int32_t* d_lookup, int64_t lookup_pitch, int32_t n_targets, double* d_pos, int64_t pos_pitch);
int tp_linpsf_fit(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images,
	const float* d_subtract, int64_t subtract_pitch,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis, int32_t max_stars,
	const int64_t* d_star_offsets, const int32_t* d_target_index,
	const double* d_pos_row, const double* d_pos_col, int64_t pos_pitch, double cutoff_radius,
	double* d_flux, double* d_flux_err, double* d_fluxes_all, int64_t out_pitch,
	double* d_contamination, int32_t* d_status, double* d_fluxes_mean);
/* tp_linpsf_flux_err: the uncertainty of the LinPSF target flux, propagated from the pixel errors.  The reference has none --
 * linpsf_photometry.py:169 writes flux_err[k] = NaN ("FIXME: Add errors!"), BasePhotometry.photometry() then refuses the light curve
 * (BasePhotometry.py:1348-1349) -- and tp_linpsf_fit keeps doing exactly that; this is a separate pass beside it, defined here.
 * For one target and one cadence k, in float64:
 *   good     = the pixels the fit uses: finite d_images value (linpsf_photometry.py:123); d_images is read for nothing else;
 *   A        = the design matrix of the fit (npx x S, linpsf_photometry.py:126-133): column s is the pixel-integrated unit PRF of
 *              fitted star s at its position of cadence k, zero outside cutoff_radius;
 *   G        = A^T A;  p = pinv(G)[t, :] with t = d_target_index and numpy's rcond = 1e-15;  m = A p (the target's flux is m . b);
 *   flux_err = sqrt(sum over good pixels of (m_px * err_px)^2), err the float32 d_images_err value widened.
 * The sum is a plain sum, as the aperture's sqrt(sum(err^2)) is (photometry.py:211): a non-finite err at a good pixel makes the
 * cadence's error NaN, also where m_px is 0.  A cadence without a good pixel gives 0 (the fit gives flux 0 there).  A target whose
 * d_target_index is not one of its fitted stars gives NaN.  A background series subtracted in the fit does not enter.
 * (Computed in one pass as W = A^T diag(err^2) A, var = p^T W p: the same number to rounding.)
 * Conventions of tp_linpsf_fit: the layouts of desc (t_pitch honoured), d_images_err laid out like d_images, d_coef / d_knots_* /
 * max_stars / d_star_offsets / d_pos_* as there, pos_pitch and out_pitch >= n_cad, d_flux_err float64 [n_targets][out_pitch] with the
 * values beyond n_cad left untouched, cutoff_radius +infinity = none.  The SPOC grid with cutoff_radius <= 5.25 runs one lane per
 * cadence out of registers (up to 8 fitted stars; 9 .. 64 out of an HBM workspace); any other grid, any radius and axes of
 * different lengths (_xy) evaluate the FITPACK box integral out of that workspace, far slower.  No atomics: two calls give the same
 * bits, and a target alone the bits it gives inside a batch. */
int tp_linpsf_flux_err_xy(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images, const float* d_images_err,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis_x, int32_t n_coef_axis_y, int32_t max_stars,
	const int64_t* d_star_offsets, const int32_t* d_target_index,
	const double* d_pos_row, const double* d_pos_col, int64_t pos_pitch, double cutoff_radius,
	double* d_flux_err, int64_t out_pitch);
int tp_linpsf_flux_err(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images, const float* d_images_err,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis, int32_t max_stars,
	const int64_t* d_star_offsets, const int32_t* d_target_index,
	const double* d_pos_row, const double* d_pos_col, int64_t pos_pitch, double cutoff_radius,
	double* d_flux_err, int64_t out_pitch);

/* ---- non-linear PSF photometry ------------------------------------------------
 * replaces PSFPhotometry.do_photometry (photometry/psf_photometry.py:111-196) with its likelihood (:52-90, statistic
 * 'Gaussian_d' with background) for a batch: per target and cadence a Nelder-Mead fit (scipy `_minimize_neldermead`, step for
 * step) of (row_stamp, column_stamp, flux) of the selected stars, warm-started from the previous cadence (the first one from
 * d_params0), then the aperture correction: flux = fitted flux + nansum(residuals in the mini aperture) (:164-171).
 *   d_images, d_backgrounds: cubes with the layout of desc (backgrounds may be NULL = 0);
 *   d_coef / d_knots_* / n_coef_axis: the PRF spline of every target, as for tp_linpsf_fit;
 *   fitted stars (ragged, CSR, at most 5 per target, the main target first: the selection of :117-136 is host catalogue work):
 *     d_star_offsets int64 [n_targets+1], d_params0 float64 [n_fit_stars][3] = (row_stamp, column_stamp, mag2flux(tmag));
 *   d_mini_aperture uint8 [n_targets][H*W]: _minimum_aperture (:29-41);
 *   variance_floor = n_readout * readnoise^2 / gain^2 (:84); maxiter_first / maxiter = 1500 / 500 upstream (:146-150);
 *   outputs float64 [n_targets][out_pitch]: d_flux, d_flux_err (NaN, :175), d_centroid_row / _col = pos_centroid[:, 0] / [:, 1]
 *     = the fitted (row_stamp, column_stamp) of the main target, as upstream (:176); a cadence whose fit did not finish within
 *     its iteration limit is NaN and does not update the starting point (:190-194);
 *   d_params_out optional float64 [n_fit_stars * 3][out_pitch] (every fitted parameter), d_nit optional int32
 *     [n_targets][out_pitch] (iterations used), d_status int32 (OK, :196).
 *   PRF grid and cutoff_radius as for tp_linpsf_fit: any grid (n = 4 .. 2048), any positive radius or +infinity; the SPOC
 *   layout with cutoff_radius <= 5.25 (PSFPhotometry uses 5, psf_photometry.py:26, :73)
 *   runs on the cached-biquartic kernel, anything else on its general instantiation (FITPACK box integral per evaluation). */
int tp_psf_fit(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images, const float* d_backgrounds,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis,
	const int64_t* d_star_offsets, const double* d_params0, const uint8_t* d_mini_aperture,
	double variance_floor, double cutoff_radius, int32_t maxiter_first, int32_t maxiter,
	double* d_flux, double* d_flux_err, double* d_centroid_row, double* d_centroid_col, int64_t out_pitch,
	double* d_params_out, int32_t* d_nit, int32_t* d_status);
/* tp_psf_flux_err: the uncertainty of the PSFPhotometry light-curve flux, propagated from the pixel errors.  The reference has none --
 * psf_photometry.py:175 writes flux_err[k] = NaN ("FIXME: Add errors!"), BasePhotometry.photometry() then refuses the light curve --
 * and tp_psf_fit keeps doing exactly that; this is a separate pass beside it, defined here.  The 'Gaussian_d'
 * likelihood is a weighted chi-square whose weights do not depend on the model, so the Gauss-Newton normal matrix at the fit's end
 * point is the Fisher information.  For one target and one cadence k, in float64 unless said otherwise:
 *   theta    = the parameters of cadence k, (row_s, col_s, f_s) of the S = min(n_fitted, 5) fitted stars, star 0 the target: d_params
 *              float64 [n_fit_stars * 3][params_pitch], the layout of tp_psf_fit's d_params_out.  A non-finite entry (the fit did not
 *              finish) gives flux_err = NaN, as does S = 0;
 *   img, w   = the fit's own float32 values, widened: var = |img + bkg| + (float)variance_floor, raised to 1e-9; w = 1 / var, raised to
 *              1e-9 (psf_photometry.py:75-86); bkg = 0 when d_backgrounds is NULL;
 *   good     = the pixels whose chi-square term the fit's nansum keeps: img and w finite;
 *   a_s(p)   = the pixel-integrated unit PRF of star s at pixel p (psf.py:122-148), zero where sqrt((j - col_s)^2 + (i - row_s)^2)
 *              >= cutoff_radius; the set of pixels inside the cut-off is frozen at theta;
 *   J        = the Jacobian of the model, good x 3S: columns f_s * da_s/drow_s, f_s * da_s/dcol_s, a_s.  The position derivatives are
 *              exact: the box integral over [e_lo, e_hi] of a spline axis has the derivative -(N(e_hi) - N(e_lo)) with respect to the
 *              star's position, N the cubic B-spline values at an edge; a limit that fpintb clips to the knot span contributes 0;
 *   N        = J^T diag(w) J;  d_i = sqrt(N_ii), 1 where that is 0;  N' = N / (d d^T);  Ninv = D^-1 pinv(N') D^-1 with numpy's rule
 *              that eigenvalues <= 1e-15 * max count as zero (N itself is badly conditioned: position and flux columns differ by
 *              the star's flux);
 *   F        = f_0 + sum over (mini aperture and good) of (img_p - mdl_p(theta)), the light-curve flux (psf_photometry.py:162-171);
 *              g = e_{f_0} - sum over (mini and good) of J_p;  q = Ninv g;  m_p = w_p (J_p . q) + [p in mini and good], the response
 *              of F to pixel p;
 *   flux_err = sqrt(sum over good pixels of (m_p * err_p)^2), err the float32 d_images_err value widened.
 * The sum is a plain sum: a non-finite err at a good pixel makes the cadence NaN, also where m_p is 0 (a flag, not arithmetic); a
 * cadence without a good pixel gives 0.  Two approximations are deliberate: the weights' own dependence on the image is ignored,
 * and the linearisation is taken at the simplex's end point as it stands (often a maxiter stop), not at the exact minimiser.
 * Conventions of tp_psf_fit: the layouts of desc (t_pitch honoured), d_backgrounds and d_images_err laid out like d_images, d_coef /
 * d_knots_* / d_star_offsets / d_mini_aperture / variance_floor / cutoff_radius as there (+infinity = no cut-off), params_pitch and
 * out_pitch >= n_cad, d_flux_err float64 [n_targets][out_pitch] with the values beyond n_cad left untouched.  One wavefront per
 * (target, cadence) and one code path for every PRF grid (the FITPACK box integral and its edge derivative); the Jacobian of a
 * cadence lives in LDS, a stamp too large for that is refused.  No atomics: two calls give the same bits, and a target alone the bits
 * it gives inside a batch. */
int tp_psf_flux_err_xy(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images, const float* d_backgrounds, const float* d_images_err,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis_x, int32_t n_coef_axis_y,
	const int64_t* d_star_offsets, const double* d_params, int64_t params_pitch, const uint8_t* d_mini_aperture,
	double variance_floor, double cutoff_radius, double* d_flux_err, int64_t out_pitch);
int tp_psf_flux_err(tp_ctx* ctx, const tp_cube_desc* desc, const float* d_images, const float* d_backgrounds, const float* d_images_err,
	const double* d_coef, const double* d_knots_x, const double* d_knots_y, int32_t n_coef_axis,
	const int64_t* d_star_offsets, const double* d_params, int64_t params_pitch, const uint8_t* d_mini_aperture,
	double variance_floor, double cutoff_radius, double* d_flux_err, int64_t out_pitch);

/* ---- light-curve diagnostics ---------------------------------------------
 * replaces the diagnostics block of BasePhotometry.photometry (photometry/BasePhotometry.py:1343-1407)
 * and utilities.rms_timescale (photometry/utilities.py:227-264) for a batch of light curves: the
 * reductions whose results the scheduler stores in its `diagnostics` table (taskmanager.py:543-563).
 *   d_flux, d_flux_err, d_centroid_col, d_centroid_row: float64 [n_targets][lc_pitch] (the outputs of
 *            tp_aperture_extract / tp_aperture_photometry);  d_time: float64 [n_cad] (days);
 *   d_quality / stride / bitmask as in tp_sumimage ("good" cadences, TESSQualityFlags.filter);
 *   d_status: optional int32 [n_targets]; only TP_STATUS_OK / TP_STATUS_WARNING targets are processed
 *            (all outputs NaN otherwise), like the `if self._status in (OK, WARNING)` of :1343;
 *   d_sumimage / d_mask (both or neither): for mask_size and edge_flux (:1394-1403);
 *   timescale_days: bin width of rms_hour (the reference uses 3600/86400);
 *   d_diag: float64 [n_targets][10] = mean_flux, variance, rms_hour, ptp, pos_centroid column, row,
 *            variability, mask_size, edge_flux, flags.  flags (as a float64 integer), a sum of the bits
 *              1  ALLNAN_FLUX    all fluxes NaN      } both ValueError upstream (:1346-1349); every light-curve
 *              2  ALLNAN_ERR     all errors NaN      } column of the row is NaN
 *              4  BAD_TIME       invalid time vector, or samples but none finite: ValueError in rms_timescale; rms_hour = NaN
 *              8  NO_DETREND     "Could not detrend ..." warning: detrend = 0 (no fitted cadence, or a rank-deficient cubic;
 *                                one fitted cadence, where the reference's polyfit fails with LinAlgError, is reported so too)
 *             16  TOO_MANY_BINS  device only: more time bins than max(n_cad, 256) on a series that is not in time order (or more
 *                                than 2e9 bins); rms_hour = NaN where the reference returns a number
 *            Light curves up to ~6 650 cadences are reduced out of LDS, longer ones (2-minute data) out of a context-owned
 *            HBM scratch with the same code.                                                                             */
int tp_lightcurve_diagnostics(tp_ctx* ctx, int32_t n_targets, int32_t n_cad,
	const double* d_flux, const double* d_flux_err, const double* d_centroid_col, const double* d_centroid_row, int64_t lc_pitch,
	const double* d_time, const int32_t* d_quality, int64_t quality_target_stride, uint32_t bitmask,
	const int32_t* d_status, const double* d_sumimage, const uint8_t* d_mask, int32_t height, int32_t width,
	double timescale_days, double* d_diag);
/* The same with a time vector per target (light curves of target pixel files: TIME is barycentric per target, so the files of a
 * group share their length and nothing else).  time_target_stride == 0: d_time is float64 [n_cad], shared -- tp_lightcurve_diagnostics
 * is this call.  Otherwise (in doubles, >= n_cad) target i reads d_time + i * time_target_stride.  A negative stride or one in
 * (0, n_cad) is TP_ERR_INVALID and nothing is written.  Same kernel, same launch, both residencies of the series (LDS / HBM
 * scratch): row i of a strided call has the bits of the shared-time call on target i alone with its own time vector.            */
int tp_lightcurve_diagnostics_times(tp_ctx* ctx, int32_t n_targets, int32_t n_cad,
	const double* d_flux, const double* d_flux_err, const double* d_centroid_col, const double* d_centroid_row, int64_t lc_pitch,
	const double* d_time, int64_t time_target_stride, const int32_t* d_quality, int64_t quality_target_stride, uint32_t bitmask,
	const int32_t* d_status, const double* d_sumimage, const uint8_t* d_mask, int32_t height, int32_t width,
	double timescale_days, double* d_diag);

/* ---- stamp cutter -----------------------------------------------------------
 * replaces BasePhotometry._load_cube, FFI branch (photometry/BasePhotometry.py:720-742), for a batch: cuts
 * every target's stamp out of a full-frame image stack resident in HBM and writes the time-fastest cube.
 *   d_frames: float32 [n_frames][frame_rows][row_pitch] (frame k at d_frames + k*frame_stride), the HDF5 group
 *             `images/%04d` (or `images_err`, `backgrounds`) of the reference loaded once per CCD;
 *   row_offset / col_offset: PIXEL_OFFSET_ROW / PIXEL_OFFSET_COLUMN (BasePhotometry.py:724-727; 0 and 44);
 *   d_stamps: int32 [n_targets][4] = (row_min, row_max, col_min, col_max) in CCD coordinates; every stamp must be
 *             desc->height x desc->width; pixels outside the frame become NaN;
 *   d_cube:   float32 cube with the layout of desc (n_cad == n_frames); the padding of the time axis (cadences n_cad ..
 *             t_pitch of every pixel) is written as zeros: the caller need not clear the cube.
 *   Layout: row_pitch >= frame_cols and frame_stride >= frame_rows * row_pitch (else rejected); only the frame_rows x frame_cols
 *   pixels of every frame are read -- d_frames may be a window of a larger stack (base pointer inside the allocation, row_pitch
 *   its full width), and what lies beside the window never reaches a cube: a stamp pixel outside the window is NaN.  No alignment
 *   of the base pointer or the pitch is assumed.  The same holds for tp_cut_stamps_multi / _masked (one geometry for all stacks)
 *   and for d_full of tp_crop_sumimage (float64, row_pitch >= frame_cols).                                        */
int tp_cut_stamps(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols,
	int64_t row_pitch, int64_t frame_stride, int32_t row_offset, int32_t col_offset,
	const int32_t* d_stamps, const tp_cube_desc* desc, float* d_cube);
/* The same for n_stacks (1 .. 4) frame stacks of one geometry at once -- the images / images_err / backgrounds groups of a CCD
 * share their stamps: one binning of the stamps, one launch.  d_frames / d_cubes: HOST arrays of n_stacks device pointers. */
int tp_cut_stamps_multi(tp_ctx* ctx, int32_t n_stacks, const float* const* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols,
	int64_t row_pitch, int64_t frame_stride, int32_t row_offset, int32_t col_offset,
	const int32_t* d_stamps, const tp_cube_desc* desc, float* const* d_cubes);
/* The same, writing only the pixel rows of every stamp's aperture mask (d_mask uint8 [n_targets][height * width], non-zero = write;
 * e.g. tp_k2p2_masks' output): tp_aperture_extract reads nothing else of the error and background cubes, and a mask is a sixth of
 * a 15 x 15 stamp on average.  The other rows of d_cubes are left as they were. */
/* The sum images of a group of stamps from the sum image of the frame (BasePhotometry.py:1001-1006: self._sumimage_full[ir1:ir2,
 * ic1:ic2]): d_out float64 [n_targets][height * width]; d_full float64 [frame_rows][row_pitch] covering the CCD rows / columns from
 * row_offset / col_offset; stamp pixels outside the frame are NaN.  d_stamps int32 [n_targets][4] as for tp_cut_stamps. */
int tp_crop_sumimage(tp_ctx* ctx, const double* d_full, int32_t frame_rows, int32_t frame_cols, int64_t row_pitch,
	int32_t row_offset, int32_t col_offset, const int32_t* d_stamps, int32_t n_targets, int32_t height, int32_t width, double* d_out);
int tp_cut_stamps_masked(tp_ctx* ctx, int32_t n_stacks, const float* const* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols,
	int64_t row_pitch, int64_t frame_stride, int32_t row_offset, int32_t col_offset,
	const int32_t* d_stamps, const tp_cube_desc* desc, const uint8_t* d_mask, float* const* d_cubes);

/* ---- the batched drop-in entry as a native job engine ----------------------------------------------------
 * replaces, for every target of a CCD region at once, what run_tessphot(_mpi).py does target by target through
 * tessphot('aperture', ...): the constructor's stamp cut (BasePhotometry._load_cube, BasePhotometry.py:720-751), the
 * catalogue of the stamp (BasePhotometry.catalog, :1094-1181), AperturePhotometry.do_photometry WITH its stamp-resize loop
 * (photometry/AperturePhotometry/photometry.py:75-170; resize_stamp / _set_stamp, BasePhotometry.py:567-693) and the
 * diagnostics of BasePhotometry.photometry (:1343-1407).  The frame stacks of the region stay in HBM; the host submits a batch
 * of targets and collects it, a worker thread of the library drives the rounds in between on streams of the engine's pool (three per slot, shared by the
 * jobs in flight, and a copy stream per slot)
 * (group by stamp size, catalogue selection, tp_cut_stamps, tp_aperture_photometry / the three stand-alone kernels for small
 * groups, tp_lightcurve_diagnostics, download, the plugin's decisions), so several jobs -- one per engine slot -- overlap.
 *
 *   tp_frames_stack: the three image groups of the region, float32 [n_frames][n_rows][n_cols] in HBM, covering CCD rows
 *     [row0, row0 + n_rows) and columns [col0, col0 + n_cols) (PIXEL_OFFSET_ROW / _COLUMN); must stay valid until the job
 *     has been waited for.
 *   tp_frames_catalog: every star of the region (host arrays, copied), binned once into cells for the per-stamp selection
 *     (stars in the stamp + its 5-pixel buffer, float32 stamp coordinates as BasePhotometry.catalog); must outlive its jobs.
 *   tp_frames_submit: host arrays (copied before it returns): targets (starid, tmag, CCD row / column), their default stamps
 *     int64 [n][4] = (row_min, row_max, col_min, col_max) and h_valid (0: "Invalid stamp selected", BasePhotometry.py:671),
 *     h_attempts (retry limit, photometry.py:70-73), h_quick_break_budget (flux_limit x expected flux for a target the
 *     haloswitch quick break applies to, NaN otherwise: photometry.py:146-158), time float64 [n_frames], quality int32
 *     [n_frames]; budget_bytes: device memory the cubes of one round may take (0: a quarter of the HBM).  Fails when every
 *     slot of the engine holds a job that has not been waited for.
 *   tp_frames_wait: joins the job (its slot is free afterwards).  Then: tp_frames_counts / _targets (per target: STATUS,
 *     final stamp, number of resizes, has_result, and where its arrays are: group, position) / _group (per device pass: its
 *     size and the page-locked host block with the layout of the packed output block -- light curves [5][n][T] float64,
 *     contamination, status, flags, mask, catalogue flags, sum image, diagnostics [n][10], each field on a 256-byte boundary)
 *     / _group_lists (catalogue CSR offsets and star ids, target ids) / _events (what the reference would have logged, as
 *     codes: 1 "No flux above threshold.", 2 / 3 minimum aperture, 4 "Too many masks.", 5 an uncaught exception of the mask
 *     stage (a = kind), 6 "Could not resize stamp any further.", 7 haloswitch quick break (value = edge flux), 8 "Too many
 *     stamp resizes.", 9 "No targets in mask.", 10 / 11 a device failure (text), 12 "Invalid stamp selected").
 *   tp_frames_release: the job's host blocks go back to the engine's pool; the job is gone.                              */
typedef struct tp_frames_engine tp_frames_engine;
typedef struct tp_frames_catalog tp_frames_catalog;
typedef struct tp_frames_job tp_frames_job;
typedef struct tp_frames_stack {
	const float* d_images;
	const float* d_images_err;
	const float* d_backgrounds;
	int32_t n_frames, n_rows, n_cols, row0, col0;
	/* optional: the sum image of the region, float64 [n_rows][n_cols] -- what the reference keeps as the HDF5 dataset
	 * 'sumimage' (prepare.py:450-453, 459; tp_frames_sumimage computes it) and BasePhotometry.sumimage crops for an FFI
	 * target (BasePhotometry.py:1001-1006).  Given, every pass takes its sum images from it (tp_crop_sumimage), builds the
	 * masks first and cuts only the in-mask pixel rows of the three stacks; NULL: the sum image of every stamp is formed from
	 * its own image cube (tp_sumimage: the reference's postage-stamp branch, BasePhotometry.py:1007-1019). */
	const double* d_sumimage;
	/* (round 6: the struct grew by the four fields below -- callers built against the older header must be recompiled; zero them
	 * for the cutting path)
	 * optional (all three or none; needs d_sumimage): the TIME-MAJOR copies of the three stacks, float32 [n_rows * n_cols][t_pitch]
	 * (tp_frames_transpose; t_pitch >= n_frames, a multiple of 4; the cadences past n_frames zero).  Given, no pass cuts anything:
	 * the extraction reads a mask pixel's time series as one row of the stack (tp_aperture_extract_stack) -- the per-target cube of
	 * BasePhotometry._load_cube (BasePhotometry.py:720-751) is never materialised.  NULL: in-mask rows are cut per pass. */
	const float* d_images_t;
	const float* d_images_err_t;
	const float* d_backgrounds_t;
	int64_t t_pitch;
} tp_frames_stack;
/* [n_frames][n_pixels] (frame_stride >= n_pixels elements from frame to frame, the elements past n_pixels never read) ->
 * d_out dense [n_pixels][t_pitch], t_pitch >= n_frames, cadences n_frames .. t_pitch of every pixel written as zeros */
int tp_frames_transpose(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride, float* d_out, int64_t t_pitch);
/* tp_aperture_extract (A6, photometry.py:172-201) with the pixels' series taken from the time-major stacks of a region: stamp
 * pixel (r, c) of target t is row (d_stamps[4 t] - stack_row0 + r) * stack_cols + d_stamps[4 t + 2] - stack_col0 + c of the
 * stacks; d_backgrounds_t NULL = aperture-only (flux_background NaN).  Same kernels and operation order as on cut cubes. */
int tp_aperture_extract_stack(tp_ctx* ctx, int32_t n_targets, int32_t n_cad, int32_t height, int32_t width,
	const float* d_images_t, const float* d_images_err_t, const float* d_backgrounds_t, int64_t t_pitch,
	int32_t stack_rows, int32_t stack_cols, int32_t stack_row0, int32_t stack_col0,
	const uint8_t* d_mask, const int32_t* d_stamps, const int32_t* d_status,
	double* d_flux, double* d_flux_err, double* d_flux_background,
	double* d_centroid_col, double* d_centroid_row, int64_t out_pitch);
int tp_frames_engine_create(int device, int32_t n_slots, tp_frames_engine** out);
int tp_frames_engine_destroy(tp_frames_engine* eng);        /* every job waited for and released first */
int tp_frames_engine_info(tp_frames_engine* eng, int32_t* n_slots, int32_t* n_free, uint64_t* hbm_bytes);
int tp_frames_catalog_create(int64_t n_stars, const int64_t* h_starid, const float* h_tmag, const double* h_row, const double* h_column,
	tp_frames_catalog** out);
int tp_frames_catalog_destroy(tp_frames_catalog* cat);
int tp_frames_submit(tp_frames_engine* eng, const tp_frames_stack* stack, const tp_frames_catalog* cat,
	int32_t n_targets, const int64_t* h_starid, const double* h_tmag, const double* h_row, const double* h_column,
	const int64_t* h_stamps, const uint8_t* h_valid, const int32_t* h_attempts, const double* h_quick_break_budget,
	const double* h_time, const int32_t* h_quality, double budget_bytes, tp_frames_job** out);
int tp_frames_wait(tp_frames_job* job);
/* has the job's worker finished (tp_frames_wait would return at once)?  A caller with several jobs in flight collects whichever
 * is done and hands its slot to the next batch. */
int tp_frames_poll(tp_frames_job* job, int32_t* done);
int tp_frames_counts(tp_frames_job* job, int32_t* n_groups, int64_t* n_events);
int tp_frames_targets(tp_frames_job* job, int32_t* status, int64_t* stamps, int32_t* stamp_resizes, uint8_t* has_result, int32_t* group, int32_t* pos);
int tp_frames_group(tp_frames_job* job, int32_t g, int32_t* n_targets, int32_t* height, int32_t* width, int64_t* cat_capacity, int64_t* n_cat,
	void** h_block, uint64_t* block_nbytes);
int tp_frames_group_lists(tp_frames_job* job, int32_t g, int64_t* cat_offsets, int64_t* cat_starid, int64_t* target_starid);
int tp_frames_events(tp_frames_job* job, int32_t* target, int32_t* code, int32_t* a, int32_t* b, double* value, int32_t* text);
const char* tp_frames_text(tp_frames_job* job, int32_t k);
int tp_frames_release(tp_frames_job* job);

/* ---- multi-GPU: the final light-curve gather (RCCL over xGMI) --------------------------------
 * replaces the pickled result messages of run_tessphot_mpi.py:114-132,163-191: targets are
 * statically sharded over the ranks (one process per GPU) and the only data-path exchange is one
 * gather of the output block.  Rank 0 obtains the 128-byte id and distributes it out of band
 * (torch.distributed store, mpi4py bcast, a file ...), then every rank calls tp_comm_init.
 * With a single rank (no tp_comm_init) gather/allgather degenerate to a device copy.           */
int tp_comm_unique_id(char* id_out, int id_len);                       /* id_len >= 128 */
int tp_comm_init(tp_ctx* ctx, const char* id, int id_len, int rank, int n_ranks);
int tp_comm_destroy(tp_ctx* ctx);
int tp_comm_info(tp_ctx* ctx, int* rank, int* n_ranks);
/* d_recv (root only) holds n_ranks * nbytes_per_rank bytes, rank r's block at r * nbytes_per_rank */
int tp_comm_gather(tp_ctx* ctx, const void* d_send, void* d_recv, uint64_t nbytes_per_rank, int root);
/* The COMPACT form of a rank's output block for the gather: the light curve's flux, flux_err and flux_background planes are
 * float32 sums widened on store (AperturePhotometry/photometry.py:172-201), so the block a rank SENDS may carry them as float32
 * and lose nothing (3 of the 5 planes halve); everything else travels as it is.  One field: `count` bytes (kind 0, copied) or
 * `count` float64 values converted to float32 (kind 1) from byte `src_offset` of the full block to byte `dst_offset` of the
 * compact one.  The layouts are the host's (photometry_amd/comm.py: packed_block_layout / compact_block_layout); rank 0 widens
 * the gathered planes again (comm.expand_blocks).  Stream-ordered on the context's stream.                                      */
typedef struct { uint64_t src_offset, dst_offset, count; int32_t kind; int32_t reserved; } tp_block_field;
int tp_block_compact(tp_ctx* ctx, const void* d_block, void* d_compact, const tp_block_field* fields, int32_t n_fields);
int tp_comm_allgather(tp_ctx* ctx, const void* d_send, void* d_recv, uint64_t nbytes_per_rank);

/* ---- image movement kernels (photometry/image_motion.py) --------------------------------------------------------------
 * tp_motion_prepare replaces ImageMovementKernel._prepare_flux (image_motion.py:74-110) for every frame of a stack
 *   d_frames float32 [n_frames] frames of [frame_rows][frame_cols] (contiguous rows) frame_stride values apart:
 *   log10(flux - nanmin + 1) rescaled to [-1, 1], the Scharr gradient magnitude of scikit-image 0.19 (mode 'reflect'),
 *   NaN -> 0.  d_out float32 [n_frames][frame_rows][frame_cols].
 * tp_motion_ecc replaces ImageMovementKernel.calc_kernel (image_motion.py:182-256): cv2.findTransformECC of every prepared
 *   frame (d_frames, as tp_motion_prepare writes them) against the prepared reference d_template [frame_rows][frame_cols],
 *   criteria (EPS | COUNT, max_iter, eps), gaussFiltSize 5, warp starting at the identity.  n_params: 2 translation,
 *   3 euclidian, 6 affine.  chunk_bytes: device memory for the blurred frames of one chunk (0: 2 GiB).  Out, per frame:
 *   d_warp float64 [n_frames][6] (w00 w01 w02 w10 w11 w12), d_rho float64 (the last correlation measured), d_iters int32 (the
 *   loop bodies run), d_status int32: 1 converged, 2 iteration cap, 3 failed (NaN correlation), 4 failed (lambda_d <= 0: the
 *   reference's calc_kernel returns NaN for 3 and 4).  Deterministic: no float atomics.                                     */
int tp_motion_prepare(tp_ctx* ctx, const float* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int64_t frame_stride,
	float* d_out);
int tp_motion_ecc(tp_ctx* ctx, const float* d_template, const float* d_frames, int32_t n_frames, int32_t frame_rows, int32_t frame_cols,
	int64_t frame_stride, int32_t n_params, int32_t max_iter, double eps, int64_t chunk_bytes, double* d_warp, double* d_rho,
	int32_t* d_iters, int32_t* d_status);

/* A loaded series of kernels applied to many positions at many times (ImageMovementKernel.load_series / interpolate / jitter,
 * image_motion.py:259-421).  The series: n_series (>= 2) finite times d_times float64, ascending, their finite kernels d_kernels
 * [n_series][P] float64 (P = 0, 2, 3, 6 for TP_MOTION_UNCHANGED, _TRANSLATION, _EUCLIDIAN, _AFFINE) and the fill kernels
 * d_fill_first / d_fill_last [P]: the first and last kernels of the series as given, finite or not.  d_query: n_times float64
 * times.  With P = 0 the three kernel pointers are not read.
 * tp_motion_interpolate: d_out [n_times][P] = scipy's interp1d(d_times, d_kernels, axis=0, assume_sorted=True,
 *   bounds_error=False, fill_value=(first, last))(d_query), operation for operation and without FMA contraction: hi =
 *   clip(searchsorted(x, t), 1, n_series - 1), lo = hi - 1, slope = (y_hi - y_lo) / (x_hi - x_lo), y = slope * (t - x_lo) + y_lo,
 *   then t < x[0] -> first, t > x[-1] -> last; a NaN time gives NaN.  Bit-defined.
 * tp_motion_star_positions: n positions d_xy [n][2] float64 (CCD column, row).  Per query time the 2 x 3 matrix M of
 *   apply_kernel (image_motion.py:113-179) is formed once; jitter = M [x y 1] - [x y] (a translation's shift and an unchanged
 *   field's zero are copies).  Position i with d_out_index[i] = o in [0, n_out) gets d_pos_col[o * pos_pitch + k] =
 *   float64(float32(d_base_col[i] + jitter column)) and the same for rows (the base columns are the float32 stamp coordinates);
 *   d_jitter (may be NULL) [n][n_times][2] float64 gets the jitter itself.  With n_out = 0 the base, index and position pointers
 *   are not read.  single = 1: the arithmetic apply_kernel does for float32 positions -- the product is rounded to float32 before
 *   the float32 position is subtracted and the base is added in float32 -- which is what catalog_attime (BasePhotometry.py:
 *   1246-1256) gets for the float32 catalogue columns; d_jitter then holds float32 values.  A position's output does not depend
 *   on the other positions of the call.                                                                                        */
#define TP_MOTION_UNCHANGED 0
#define TP_MOTION_TRANSLATION 1
#define TP_MOTION_EUCLIDIAN 2
#define TP_MOTION_AFFINE 3
int tp_motion_interpolate(tp_ctx* ctx, int32_t warpmode, int32_t n_series, const double* d_times, const double* d_kernels,
	const double* d_fill_first, const double* d_fill_last, int32_t n_times, const double* d_query, double* d_out);
int tp_motion_star_positions(tp_ctx* ctx, int32_t warpmode, int32_t n_series, const double* d_times, const double* d_kernels,
	const double* d_fill_first, const double* d_fill_last, int32_t n_times, const double* d_query, int64_t n, const double* d_xy,
	int32_t single, const float* d_base_col, const float* d_base_row, const int64_t* d_out_index, int64_t n_out, double* d_pos_col,
	double* d_pos_row, int64_t pos_pitch, double* d_jitter);

/* ---- Halo photometry (photometry/halo/halo_photometry.py; csrc/halo.hip, its rules in csrc/halo_rules.h) --------------------
 * The TV-min pixel weights that halo_photometry.py:179-196 obtains from halophot's do_lc (settings of :86-97: objective 'tv',
 * sub 1, thresh -1, no sigma clipping, uniform start), defined in DESIGN.md ("Halo") and tests/halo_common.py.  One problem is
 * one light-curve segment of one target (the split times of :125-159).
 *   h_p_offset, h_npix, h_ncad: HOST arrays [n_problems].  Problem i's pixel matrix is ncad[i] rows of round_up(npix[i], 4)
 *   floats (zero padded) at d_P + p_offset[i] (p_offset a multiple of 4, d_P 16-byte aligned): row t holds the cube's float32
 *   values of the npix pixels at cadence t, every one of them finite.  1 <= npix <= 4096.  d_fit uint8 [sum ncad]: non-zero
 *   for a fitted cadence (quality & DEFAULT_BITMASK == 0), problem i's cadences after those of problems 0 .. i-1.
 *   Weights w = softmax(theta), l_t = sum_p w_p P[t][p] (float64), f = sum |l_F[j+1] - l_F[j]| / median(l_F) over the fitted
 *   cadences F in time order (numpy's median).  Fewer than 3 fitted cadences, or a median <= 0 / not finite at the start:
 *   status 4 (degenerate), f NaN.
 * tp_halo_tvmin minimises f over theta from theta = 0: L-BFGS with `history` pairs (<= 16; the reference's setting is 10),
 *   backtracking Armijo line search (alpha = 1, c1 = 1e-4, halving, 20 trials), stop after maxiter iterations (status 2), when
 *   f_k - f_k+1 <= ftol max(|f_k|, |f_k+1|, 1) or |grad theta|_inf <= gtol (status 1), or when the line search fails (status 3).
 *   Out: d_w float64 [sum npix] (weights, problem i after problems 0 .. i-1), d_l float64 [sum ncad] (l at every cadence of the
 *   problem, fitted or not), d_f float64 [n_problems], d_iters int32, d_status int32.
 * tp_halo_objective: f (d_f [n_problems]) and its gradient with respect to theta (d_grad float64 [sum npix]) at d_theta
 *   (float64 [sum npix]), one evaluation per problem; NaN for a degenerate problem.
 * Both are deterministic (no float atomics): a problem gives the same bits alone as inside a batch.                          */
int tp_halo_tvmin(tp_ctx* ctx, int32_t n_problems, const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad,
	const float* d_P, const uint8_t* d_fit, int32_t maxiter, int32_t history, double ftol, double gtol, double* d_w, double* d_l,
	double* d_f, int32_t* d_iters, int32_t* d_status);
int tp_halo_objective(tp_ctx* ctx, int32_t n_problems, const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad,
	const float* d_P, const uint8_t* d_fit, const double* d_theta, double* d_f, double* d_grad);

/* ---- Halo photometry of a batch of targets straight from a region's frame stack (the batched entry; csrc/halo_stack.hip) ----
 * The problems of halo_photometry.py:160-196 (one per segment of every target; the definition is tests/halo_common.py::problems)
 * are built on the device from the image-major stack d_images float32 [n_frames][frame_rows][frame_cols] (contiguous) that covers
 * the CCD rows / columns from row0 / col0.  h_stamps: HOST int32 [n_targets][4] (row1, row2, col1, col2 in CCD coordinates), all
 * of height x width (<= 4096 pixels) and inside the stack.  h_seg: HOST int32 [n_frames], the segment of every cadence (-1: no
 * finite time), n_seg = its largest value + 1 (1 .. 64).  Problem q = target * n_seg + segment.
 * tp_halo_select_stack: d_mask uint8 [n_targets][height * width] the pixel mask (:118-120), h_quality HOST int32 [n_frames]; a
 *   cadence is fitted iff quality & bitmask == 0.  A mask pixel is dropped iff nanmedian (float64) of its float32 values over the
 *   segment's fitted cadences is < minflux (NaN medians keep it); a cadence of the segment is kept iff every kept pixel is finite
 *   there (all of them when no pixel is kept).  Out: d_pix int32 [n_prob][height * width] (flat stamp indices, ascending, the
 *   first d_npix[q]), d_cad int32 [n_prob][n_frames] (ascending, the first d_ncad[q]), d_fit uint8 [n_prob][n_frames] (the fit flag
 *   of every kept cadence), d_cadpos int32 [n_targets][n_frames] (position of the cadence in its problem's list, -1: in none),
 *   d_npix / d_ncad int32 [n_prob].
 * tp_halo_gather_stack: for the n_run problems h_index (HOST, indices q) with their counts h_npix / h_ncad (HOST, as read back from
 *   tp_halo_select_stack; 1 <= npix) and offsets h_p_offset (HOST, multiples of 4): d_P in tp_halo_tvmin's layout (zero padded rows)
 *   and d_fit_out uint8 [sum ncad], problem r's cadences after those of problems 0 .. r-1.
 * tp_halo_outputs_stack (:197-219): from d_w / d_l / d_status of tp_halo_tvmin over the same n_run problems and d_images_err (the
 *   region's error stack): d_median float64 [n_prob] numpy's median of l over the fitted cadences (NaN for a problem not run);
 *   d_weightmap float64 [n_prob][height * width] = w / median at the kept pixels, zero elsewhere; d_corr float64 [n_targets][n_frames]
 *   = l / median at the problem's cadences, NaN elsewhere and for a degenerate problem; d_flux = d_corr * h_normfactor[target];
 *   d_flux_err = |normfactor| sqrt(nansum(weightmap^2 err^2)) over the stamp with the weight map of the cadence's segment, 0 for a
 *   cadence without one.  Every sum has a fixed order and nothing uses float atomics: results are bit-reproducible and a target
 *   gives the same bits alone as inside a batch.                                                                              */
int tp_halo_select_stack(tp_ctx* ctx, const float* d_images, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int32_t row0,
	int32_t col0, int32_t n_targets, const int32_t* h_stamps, int32_t height, int32_t width, const uint8_t* d_mask, int32_t n_seg,
	const int32_t* h_seg, const int32_t* h_quality, int32_t bitmask, double minflux, int32_t* d_pix, int32_t* d_cad, uint8_t* d_fit,
	int32_t* d_cadpos, int32_t* d_npix, int32_t* d_ncad);
int tp_halo_gather_stack(tp_ctx* ctx, const float* d_images, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int32_t row0,
	int32_t col0, int32_t n_targets, const int32_t* h_stamps, int32_t height, int32_t width, int32_t n_seg, const int32_t* d_pix,
	const int32_t* d_cad, const uint8_t* d_fit, int32_t n_run, const int32_t* h_index, const int64_t* h_p_offset, const int32_t* h_npix,
	const int32_t* h_ncad, float* d_P, uint8_t* d_fit_out);
int tp_halo_outputs_stack(tp_ctx* ctx, const float* d_images_err, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int32_t row0,
	int32_t col0, int32_t n_targets, const int32_t* h_stamps, int32_t height, int32_t width, int32_t n_seg, const int32_t* h_seg,
	const int32_t* d_pix, const int32_t* d_cadpos, int32_t n_run, const int32_t* h_index, const int32_t* h_npix, const int32_t* h_ncad,
	const uint8_t* d_fit, const double* d_w, const double* d_l, const int32_t* d_status, const double* h_normfactor, double* d_median,
	double* d_corr, double* d_flux, double* d_flux_err, double* d_weightmap);

/* ---- Halo photometry of a group of target pixel files straight from their stamp cubes (csrc/halo_cubes.hip) ------------------
 * The same problems, rules and outputs as the _stack entries above, for targets that share a stamp shape and a number of cadences
 * and nothing else.  d_images / d_images_err: float32 [n_targets][height * width][t_pitch], time fastest, t_pitch >= n_cad (the
 * pads are never read); height * width <= 4096.  Every target has its own segments: h_prob_off HOST int32 [n_targets + 1], rising
 * from 0 by 1 .. 64 per target; problem q = h_prob_off[i] + k is segment k of target i, n_prob = h_prob_off[n_targets] (<= 65535).
 * h_seg HOST int32 [n_targets][n_cad]: the segment of every cadence of every target, -1 .. n_seg_i - 1 in row i (-1: none; anything
 * else is rejected); h_quality HOST int32 [n_targets][n_cad].
 * tp_halo_select_cubes: d_mask uint8 [n_targets][height * width]; the pixel and cadence rules of tp_halo_select_stack per problem (a
 *   segment without a cadence keeps every mask pixel).  Out: d_pix int32 [n_prob][height * width], d_cad int32 [n_prob][n_cad],
 *   d_fit uint8 [n_prob][n_cad], d_cadpos int32 [n_targets][n_cad], d_npix / d_ncad int32 [n_prob], as there.
 * tp_halo_gather_cubes: the n_run problems h_index with h_npix / h_ncad / h_p_offset (HOST, as for tp_halo_gather_stack): d_P in
 *   tp_halo_tvmin's layout (zero padded rows) and d_fit_out uint8 [sum ncad].
 * tp_halo_outputs_cubes: d_median float64 [n_prob], d_weightmap float64 [n_prob][height * width], d_corr / d_flux / d_flux_err
 *   float64 [n_targets][n_cad], defined as for tp_halo_outputs_stack; the sum of d_flux_err runs over the stamp's pixels in ascending
 *   order in the grouping of numpy's pairwise sum, NaN terms counting as 0, and is 0 for a cadence without a segment.
 * Nothing uses float atomics: results are bit-reproducible, and a target gives the same bits alone, in a batch and in any chunking. */
int tp_halo_select_cubes(tp_ctx* ctx, const float* d_images, int32_t n_targets, int32_t height, int32_t width, int32_t n_cad, int32_t t_pitch,
	const uint8_t* d_mask, const int32_t* h_prob_off, const int32_t* h_seg, const int32_t* h_quality, int32_t bitmask, double minflux,
	int32_t* d_pix, int32_t* d_cad, uint8_t* d_fit, int32_t* d_cadpos, int32_t* d_npix, int32_t* d_ncad);
int tp_halo_gather_cubes(tp_ctx* ctx, const float* d_images, int32_t n_targets, int32_t height, int32_t width, int32_t n_cad, int32_t t_pitch,
	const int32_t* h_prob_off, const int32_t* d_pix, const int32_t* d_cad, const uint8_t* d_fit, int32_t n_run, const int32_t* h_index,
	const int64_t* h_p_offset, const int32_t* h_npix, const int32_t* h_ncad, float* d_P, uint8_t* d_fit_out);
int tp_halo_outputs_cubes(tp_ctx* ctx, const float* d_images_err, int32_t n_targets, int32_t height, int32_t width, int32_t n_cad, int32_t t_pitch,
	const int32_t* h_prob_off, const int32_t* h_seg, const int32_t* d_pix, const int32_t* d_cadpos, int32_t n_run, const int32_t* h_index,
	const int32_t* h_npix, const int32_t* h_ncad, const uint8_t* d_fit, const double* d_w, const double* d_l, const int32_t* d_status,
	const double* h_normfactor, double* d_median, double* d_corr, double* d_flux, double* d_flux_err, double* d_weightmap);

/* ---- TAN-SIP world coordinate systems (astropy.wcs as ImageMovementKernel('wcs') uses it, image_motion.py:113-421) ---------
 * One frame's WCS is a block of TP_WCS_PARAMS float64 values packed by photometry_amd/wcs.py: [0:9] the native -> celestial
 * rotation (row-major), [9:11] CRPIX, [11:15] CD, [15:19] CD^-1, [19] A_ORDER, [20] B_ORDER, [21] 1 with SIP, [24:124] A_p_q at
 * p * 10 + q, [124:224] B_p_q.  All arithmetic is float64; nothing uses float atomics, so every result is bit-reproducible.
 * tp_wcs_pix2world: n points d_xy [n][2] (x, y; `origin` 0 or 1) of one frame: mode 0 pix2foc, 1 wcs_pix2world (no SIP),
 *   2 all_pix2world.  d_out [n][2] (focal-plane pixels, or ra in [0, 360) and dec in degrees; may be NULL for modes 1 and 2),
 *   d_cos [n][3] the celestial unit vectors (modes 1 and 2; may be NULL).
 * tp_wcs_radec: (ra, dec) degrees d_radec [n][2] -> unit vectors d_cos [n][3].
 * tp_wcs_world2pix: the points d_cos [n][3] in every frame of d_params [n_frames][TP_WCS_PARAMS] (<= 65535); the points form
 *   n_batches batches, h_offsets (HOST, [n_batches + 1], rising from >= 0 to <= n).  all = 0: wcs_world2pix; all = 1:
 *   all_world2pix (astropy 4.3, adaptive=False, detect_divergence=True) with `tolerance` and `maxiter`, the loop's stopping test
 *   taken over each batch.  d_pix [n_frames][n][2] (`origin`), d_status [n_frames][n] TP_WCS_* bits, d_iters [n_frames][n_batches]
 *   (astropy's k, 0 without SIP or for an empty batch; may be NULL).  Empty batches are allowed (d_cos may be NULL when n == 0).
 * tp_wcs_footprint_check: load_series' test of every frame: pixel (0, 0) through all_pix2world and back through all_world2pix as a
 *   batch of one; d_status [n_frames] TP_WCS_* bits (0: the frame is kept).
 * tp_wcs_star_positions: LinPSF positions of catalogue rows that move with the WCS.  Rows d_xy32 [n][2] (column, row float32, in
 *   the reference WCS d_ref_params), batches h_offsets (HOST) as in tp_wcs_world2pix -- a stamp's catalogue.  Per cadence k the
 *   jitter is that of frame d_k1[k] (d_k2[k] = -1) or interp1d's (j2 - j1) / dt[k] * dx[k] + j1 between frames k1 and k2; row i
 *   with d_out_index[i] = o >= 0 (< n_out) gets d_pos_col[o * pos_pitch + k] = float64(float32(base_col[i] + jitter column)),
 *   the same for rows.  d_status [n] (may be NULL): OR of the rows' status bits over the cadences (atomic integer OR).        */
#define TP_WCS_PARAMS 224
#define TP_WCS_DIVERGENT 1   /* astropy's `divergent` points (invalid ones included) */
#define TP_WCS_SLOW 2        /* maxiter reached while still converging */
#define TP_WCS_INVALID 4     /* non-finite pixel from a finite world point */
#define TP_WCS_SCHEDULE 8    /* batch of > 64 points: dn rose above tolerance^2 again after the point had converged; the batch's
                                iteration count and its other points may then differ from astropy's (see csrc/wcs.hip) */
int tp_wcs_pix2world(tp_ctx* ctx, const double* d_params, int64_t n, const double* d_xy, int32_t origin, int32_t mode, double* d_out,
	double* d_cos);
int tp_wcs_radec(tp_ctx* ctx, int64_t n, const double* d_radec, double* d_cos);
int tp_wcs_world2pix(tp_ctx* ctx, const double* d_params, int32_t n_frames, int64_t n, int32_t n_batches, const int64_t* h_offsets,
	const double* d_cos, int32_t origin, int32_t all, double tolerance, int32_t maxiter, double* d_pix, int32_t* d_status, int32_t* d_iters);
int tp_wcs_footprint_check(tp_ctx* ctx, const double* d_params, int32_t n_frames, double tolerance, int32_t maxiter, int32_t* d_status);
int tp_wcs_star_positions(tp_ctx* ctx, const double* d_params, int32_t n_frames, const double* d_ref_params, int64_t n, int32_t n_batches,
	const int64_t* h_offsets, const float* d_xy32, const float* d_base_col, const float* d_base_row, const int64_t* d_out_index, int64_t n_out,
	int32_t n_cad, const int32_t* d_k1, const int32_t* d_k2, const double* d_dt, const double* d_dx, double tolerance, int32_t maxiter,
	double* d_pos_col, double* d_pos_row, int64_t pos_pitch, int32_t* d_status);

/* ---- FITS image data units (csrc/fitsin.hip; the rules in csrc/fits_rules.h) -------------------------------------------------
 * What FFIImage does with astropy on the host -- `np.asarray(hdu[1].data[0:2048, 44:2092], dtype='float32')` and the same for the
 * uncertainty HDU (io.py:46-48), or the whole image of HDU 0 / 1 for other files (io.py:80-82) -- on a data unit that lies in device
 * memory byte for byte as in the file (big-endian, NAXIS1 fastest).
 * tp_fits_unpack: the window [row0, row0 + rows) x [col0, col0 + cols) of the naxis2 x naxis1 image at d_raw (16-byte aligned; the
 *   host layer puts a unit on a 256-byte boundary) into d_out [rows][out_row_pitch] float32 (out_row_pitch >= cols, in values; what
 *   lies between two rows is never written).  bitpix -32: the bytes of every value swapped, nothing else -- NaN payloads, +-inf,
 *   -0.0 and denormals keep their bits.  bitpix -64: swapped, then float64 -> float32 rounded to nearest even like a C cast / numpy's
 *   astype (denormal results kept, overflow to inf, NaN quiet with the top of its payload).  Rows whose 16-byte boundaries agree
 *   between file and output move as 16-byte loads and stores with single values before and after (the TESS science window: all
 *   of it), any other geometry value by value.  Any other bitpix (integer images, BSCALE / BZERO), a window that leaves the image
 *   or is empty, a pitch below cols, a misaligned pointer: TP_ERR_INVALID and nothing is written.
 * tp_fits_datasum: the DATASUM of the FITS checksum convention for the nbytes (a multiple of 4, < 2^34; a data unit with its
 *   padding) at d_raw (16-byte aligned): the ones'-complement sum of the big-endian 32-bit words, i.e. their 64-bit integer sum with
 *   the carries folded back, in d_wordsum[0] (device, 8-byte aligned).  Integer atomics only: the result is exact and
 *   the same in every run.
 * Both are asynchronous on the context's stream.                                                                                */
int tp_fits_unpack(tp_ctx* ctx, const void* d_raw, int32_t bitpix, int32_t naxis1, int32_t naxis2, int32_t row0, int32_t col0, int32_t rows,
	int32_t cols, float* d_out, int64_t out_row_pitch);
int tp_fits_datasum(tp_ctx* ctx, const void* d_raw, uint64_t nbytes, uint64_t* d_wordsum);

/* ---- target pixel files (csrc/tpfin.hip; the rules in csrc/tpf_rules.h) ---------------------------------------------------------
 * What BasePhotometry._load_cube does with astropy on the host for a `tpf` run -- `cube[:, :, k] = data[field][k]` for every row k
 * of the PIXELS table (BasePhotometry.py:720-751) -- on the table's data unit as it lies in device memory byte for byte as in the
 * file: n_rows rows of row_bytes bytes, one cadence per row, big-endian.
 * tp_tpf_unpack: n_cols (1..4) image columns of TFORM `E` (big-endian float32, n_pix values each, beginning h_col_offsets[c] bytes
 *   into a row; HOST array) into the cubes h_d_out[c] (HOST array of device pointers), each [n_pix][t_pitch] float32 with the
 *   cadence fastest and the pixels in the row's own order (TDIM lists the fastest axis first: pixel = r * W + c).  h_rows (HOST;
 *   may be NULL: all rows, T == n_rows): the T table rows that are kept, strictly increasing -- the reference drops the rows whose
 *   TIME is not finite (BasePhotometry.py:339-340); the list is checked before anything is queued.  The bytes of every value are
 *   swapped and nothing else: NaN payloads, signalling NaNs, -0.0 and denormals keep their bits.  The pad cadences [T, t_pitch) of
 *   every pixel are written as 0.0, so the cubes need no memset.  One launch for all columns.
 *   TP_ERR_INVALID and nothing written: a null pointer, d_table or a cube not 4-byte aligned, row_bytes or a column offset that
 *   is no multiple of 4, a column that leaves the row (offset + 4 * n_pix > row_bytes), n_cols outside [1, 4], n_pix outside
 *   [1, 2^22], n_rows outside [1, 2^31), n_rows * row_bytes at or above 2^34 (the bound of tp_fits_datasum, which checks the table's
 *   DATASUM), T outside [1, n_rows], t_pitch below T or no multiple of 32, a row list that is out of range or does not rise.
 * Asynchronous on the context's stream.                                                                                        */
int tp_tpf_unpack(tp_ctx* ctx, const void* d_table, int64_t row_bytes, int64_t n_rows, const int32_t* h_rows, int64_t T, int32_t n_cols,
	const int64_t* h_col_offsets, int64_t n_pix, float* const* h_d_out, int64_t t_pitch);

/* ---- per-stamp flag series (csrc/stampflags.hip; the rules in csrc/stampflags_rules.h) ------------------------------------------
 * What save_lightcurve does on the host for one target -- `quality[np.any(self.pixelflags_cube & PixelQualityFlags.BackgroundShenanigans
 * != 0, axis=(0, 1))] |= CorrectorQualityFlags.BackgroundShenanigans` (BasePhotometry.py:1445-1449) -- for every target of a batch in
 * one launch, on the region's pixel-flag stack d_flags: uint8, n_frames frames of frame_rows x frame_cols pixels (columns fastest),
 * frame_stride bytes from one frame to the next, covering CCD rows [row0, row0 + frame_rows) and columns [col0, col0 + frame_cols).
 * tp_stamp_flag_series: h_stamps (HOST, [n_targets][4]: r1, r2, c1, c2 in CCD pixels, rows [r1, r2), columns [c1, c2)) are the
 *   targets' stamps.  d_out[i * out_pitch + t] = out_value when any pixel of stamp i in frame t has `flags & flag_mask != 0`, else 0,
 *   for t in [0, n_frames); [n_frames, out_pitch) of a row is never written.  A stamp of (-1, -1, -1, -1) -- a target without a
 *   stamp -- gives a row of zeros.  Integers: the result is exact and the same in every run.
 *   TP_ERR_INVALID, checked on the host before anything is queued, nothing written: a stamp that leaves the frames or has r2 <= r1 or
 *   c2 <= c1 (other than the all -1 form), a null pointer, d_out not 4-byte aligned, flag_mask == 0, n_frames < 1, n_targets < 1,
 *   out_pitch < n_frames, frame_stride < frame_rows * frame_cols, a frame of 2^31 pixels or more, ceil(n_frames / 16) *
 *   ceil(n_targets / 4) at or above 2^31.
 * Asynchronous on the context's stream; one launch per call.                                                                     */
int tp_stamp_flag_series(tp_ctx* ctx, const uint8_t* d_flags, int32_t n_frames, int32_t frame_rows, int32_t frame_cols, int64_t frame_stride,
	int32_t row0, int32_t col0, int32_t n_targets, const int64_t* h_stamps, uint32_t flag_mask, int32_t out_value, int32_t* d_out, int64_t out_pitch);

/* ---- batched DEFLATE (csrc/deflate.hip; the rules in csrc/deflate_rules.h) -----------------------------------------------------------
 * RFC 1951 on the device, for the gzip members of the light-curve files.  The n_streams streams of a call lie in d_in: stream s is
 * d_in[off[s], off[s + 1]) with off = h_stream_offsets (HOST, n_streams + 1 values that do not fall).  A stream is cut into chunks of
 * tp_deflate_chunk_bytes() input bytes, the last one shorter, a stream of 0 bytes has none; the chunks of a call are numbered in call
 * order.  Every chunk has a window of its own and becomes a byte-aligned run of complete blocks without BFINAL (dynamic, fixed or
 * stored, whichever is smallest; a coded block is followed by an empty stored block), so the outputs of a stream's chunks,
 * concatenated, followed by the two bytes 03 00, are a raw deflate stream of the stream's bytes.
 * tp_deflate: d_out receives the outputs of all chunks back to back; d_chunk_end[c] (uint64) is the offset in d_out at which chunk c
 *   ends, d_chunk_crc[c] the CRC-32 (gzip polynomial) of its input bytes.  Bytes of d_out behind the last end are never written.  The
 *   output is a function of the input bytes alone: the same in every run.  d_work: scratch of tp_deflate_work_bytes(off, n_streams)
 *   bytes, in use until the call's work on the stream is over.  Alignments: d_in and d_out none, d_chunk_end 8, d_chunk_crc 4, d_work 16.
 *   TP_ERR_INVALID, checked on the host before anything is queued, nothing written: a null pointer with work to do, offsets that
 *   fall, n_streams < 1, 2^34 bytes or more in all, out_capacity below the sum of tp_deflate_bound over the streams, work_bytes
 *   below tp_deflate_work_bytes, a misaligned pointer.  A call without a byte of input queues nothing and reads no pointer.
 *   Asynchronous on the context's stream; three launches per call (encode, running ends, pack).
 * tp_deflate_bound(nbytes): the most output bytes of a stream of nbytes bytes: nbytes + 5 per chunk (the stored form).
 * tp_deflate_work_bytes: the scratch of a call, 0 for arguments tp_deflate refuses.  tp_deflate_chunk_bytes: the chunk length.
 * tp_crc32_combine: crc(A || B) from crc(A), crc(B) and len(B), so that a stream's CRC follows from its chunks'.
 * The last four are host-only and need no context.                                                                               */
int tp_deflate(tp_ctx* ctx, const void* d_in, const uint64_t* h_stream_offsets, int64_t n_streams, void* d_out, uint64_t out_capacity,
	uint64_t* d_chunk_end, uint32_t* d_chunk_crc, void* d_work, uint64_t work_bytes);
uint64_t tp_deflate_bound(uint64_t nbytes);
uint64_t tp_deflate_work_bytes(const uint64_t* h_stream_offsets, int64_t n_streams);
uint64_t tp_deflate_chunk_bytes(void);
uint32_t tp_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* ---- batched INFLATE (csrc/inflate.hip; the rules in csrc/inflate_rules.h) -----------------------------------------------------------
 * RFC 1951 decoded on the device, for gzip files read as they lie on disk.  The n_streams streams of a call are raw deflate streams
 * (the gzip framing is host work): stream s is d_in[in[s], in[s + 1]) with in = h_in_offsets, and may write its slot
 * d_out[o[s], o[s + 1]) with o = h_out_offsets (both HOST, n_streams + 1 values that do not fall).  One wavefront decodes a stream.
 * tp_inflate: per stream s, d_status[s] is one of TP_INFLATE_*, d_out_bytes[s] the bytes produced (they lie at the front of the slot),
 *   d_in_bytes[s] the bytes consumed up to the last bit of the block with BFINAL -- what lies behind it in the stream is not read --
 *   and d_crc[s] the CRC-32 (gzip polynomial) of the bytes produced, formed on the device.  Acceptance is zlib's: the status is
 *   TP_INFLATE_OK exactly where zlib's inflate reaches the end of the stream, and then bytes, consumed count and CRC are zlib's.  A
 *   stream whose status is not TP_INFLATE_OK never makes the call fail: it has its status, the bytes it produced before the rule broke
 *   (counted and summed; d_in_bytes[s] is then the stream's length), and has written nothing outside its slot.  Bytes of a slot behind
 *   the bytes produced are never written.  The results are a function of the input bytes and the slot sizes alone.
 *   Alignments: d_in and d_out none, d_status 4, d_out_bytes 8, d_in_bytes 8, d_crc 4.
 *   TP_ERR_INVALID, checked on the host before anything is queued, nothing written: a null result or offset pointer, d_in null with
 *   input bytes or d_out null with slot bytes, offsets that fall, n_streams < 1, 2^34 bytes or more of input or of slots, a
 *   misaligned result pointer.
 *   Asynchronous on the context's stream; one launch per call.                                                                    */
enum tp_inflate_status {
	TP_INFLATE_OK = 0,
	TP_INFLATE_INPUT_ENDS = 1,        /* a bit behind the stream's last byte was needed */
	TP_INFLATE_BAD_BLOCK_TYPE = 2,    /* BTYPE 3 */
	TP_INFLATE_STORED_LENGTH = 3,     /* LEN != ~NLEN */
	TP_INFLATE_TOO_MANY_SYMBOLS = 4,  /* HLIT > 286 or HDIST > 30 */
	TP_INFLATE_BAD_CODE_LENGTHS = 5,  /* over-subscribed or incomplete code, symbol 16 first, a repeat past HLIT + HDIST */
	TP_INFLATE_NO_END_OF_BLOCK = 6,   /* len[256] == 0 */
	TP_INFLATE_BAD_SYMBOL = 7,        /* bits that are no code, length symbol 286 / 287, distance symbol 30 / 31 */
	TP_INFLATE_DISTANCE_TOO_FAR = 8,  /* a distance beyond the bytes produced */
	TP_INFLATE_OUTPUT_FULL = 9        /* the slot is smaller than the content */
};
int tp_inflate(tp_ctx* ctx, const void* d_in, const uint64_t* h_in_offsets, int64_t n_streams, void* d_out, const uint64_t* h_out_offsets,
	int32_t* d_status, uint64_t* d_out_bytes, uint64_t* d_in_bytes, uint32_t* d_crc);

/* ---- light-curve table out (csrc/lctable.hip; the rules in csrc/lctable_rules.h) ---------------------------------------------------
 * What fitsio.bintable_hdu does on the host for the LIGHTCURVE table of a light-curve file (FILEVER 1.5; BasePhotometry.py:1507-1600) --
 * the recarray fill, `tobytes`, the pad and the DATASUM -- from the planes a run holds in device memory.  A row is 96 bytes, big-endian,
 * 14 columns `D E J D D D D D J J D D D D`: TIME, TIMECORR, CADENCENO, FLUX_RAW, FLUX_RAW_ERR, FLUX_BKG, FLUX_CORR, FLUX_CORR_ERR,
 * QUALITY, PIXEL_QUALITY, MOM_CENTR1, MOM_CENTR2, POS_CORR1, POS_CORR2.
 * tp_lc_table_src: the source of a call.  Every pointer is a device pointer; every stride is in elements; a per-target stride of 0 is
 *   one vector shared by all targets.  time, timecorr (float64), cadenceno, pixel_quality (int32): value of target i at cadence t at
 *   [i * stride + t].  lc: the five float64 planes flux, flux_err, flux_background, centroid column, centroid row, value at
 *   [p * lc_plane_stride + i * lc_target_stride + t] (the (5, m, T) block of the frames entry: m * T and T).  quality: int32
 *   [i * stride + t], NULL: zeros.  pos_corr: float64 [i * stride + 2 * t + {0, 1}], NULL: zeros.
 * tp_lc_table_pack: for target i in [0, n_targets) the n_rows rows of the cadences d_rows[0 .. n_rows) (device int32, rising, each in
 *   [0, T); NULL: 0 .. n_rows - 1) at d_out + h_out_offsets[i] (HOST array), then zeros up to the next multiple of 2880 bytes; no
 *   other byte of d_out is written.  The float64 columns move as 64-bit integers and are byte-swapped only: a NaN keeps payload and
 *   sign, -0.0 stays -0.0, a signalling NaN stays signalling.  TIMECORR is the float32 nearest to the value, ties to even (numpy's
 *   assignment into an '>f4' field).  FLUX_CORR and FLUX_CORR_ERR are the bits of np.nan, 0x7FF8000000000000.  An entry of d_rows
 *   outside [0, T) reads nothing: its row is written from zeros.  d_datasum[i] (uint64, 8-byte aligned): the DATASUM of target i's data
 *   unit in the form tp_fits_datasum returns, from the native values on the way (no written byte is read back; integer atomics only:
 *   exact and the same in every run).  n_rows == 0 writes no byte of d_out and sets the sums to 0.
 *   TP_ERR_INVALID, checked on the host before anything is queued, nothing written: a null pointer other than d_rows, quality and
 *   pos_corr, n_targets outside [1, 2^20], T outside [1, 2^31), n_rows outside [0, T] or above 178 956 970 (kMaxRows of the rules: beyond
 *   it the 64-bit word sum could wrap), a negative stride, d_out not 16-byte aligned, an offset that is no multiple of 16, a target's
 *   range that leaves out_capacity, two ranges that overlap, d_datasum not 8-byte or d_rows not 4-byte aligned.
 *   Asynchronous on the context's stream; two launches per call (pack, fold).
 * tp_lc_place: n_segments byte ranges in one launch: h_lengths[k] bytes from d_src + h_src_offsets[k] to d_dst + h_dst_offsets[k] (HOST
 *   arrays; all three multiples of 16 -- every FITS piece is a multiple of 2880), for the host-built pieces of a window of files after
 *   one compact upload.  TP_ERR_INVALID, nothing written: a null pointer, n_segments outside [1, 2^20], a value or a buffer that is not
 *   16-byte aligned, a range that leaves src_capacity or dst_capacity, destination ranges that overlap, 2^34 bytes or more in all.
 *   Asynchronous on the context's stream; one launch per call (none without a byte to move).                                       */
typedef struct tp_lc_table_src {
	const double* time; int64_t time_stride;
	const double* timecorr; int64_t timecorr_stride;
	const int32_t* cadenceno; int64_t cadenceno_stride;
	const int32_t* pixel_quality; int64_t pixel_quality_stride;
	const double* lc; int64_t lc_plane_stride; int64_t lc_target_stride;
	const int32_t* quality; int64_t quality_stride;
	const double* pos_corr; int64_t pos_corr_stride;
} tp_lc_table_src;
int tp_lc_table_pack(tp_ctx* ctx, const tp_lc_table_src* h_src, const int32_t* d_rows, int64_t n_rows, int64_t T, int32_t n_targets, void* d_out,
	const uint64_t* h_out_offsets, uint64_t out_capacity, uint64_t* d_datasum);
int tp_lc_place(tp_ctx* ctx, const void* d_src, uint64_t src_capacity, const uint64_t* h_src_offsets, const uint64_t* h_dst_offsets, const uint64_t* h_lengths,
	int64_t n_segments, void* d_dst, uint64_t dst_capacity);

/* ---- synthetic data (bench / test utility, not part of the reference path) -----------------
 * Fill images / images_err / backgrounds cubes on the device from scene parameters, following
 * the data model of simulation/simulateFITS.py:338-405 (see photometry_amd/simulate.py).
 *   d_star_params: float64 [n_targets][n_slots][3] = (row_stamp, col_stamp, flux); flux 0 = unused
 *   d_sigma_psf, d_bkg_level, d_bkg_phase: float64 [n_targets]
 *   d_jitter: float64 [n_cad][2] (column, row) per-cadence shift
 *   any of d_images / d_images_err / d_backgrounds / d_raw may be NULL.                        */
int tp_synth_fill(tp_ctx* ctx, const tp_cube_desc* desc, int32_t n_slots,
	const double* d_star_params, const double* d_sigma_psf, const double* d_bkg_level,
	const double* d_bkg_phase, const double* d_jitter, double readnoise, double nan_fraction,
	uint64_t seed, float* d_images, float* d_images_err, float* d_backgrounds, float* d_raw);

#ifdef __cplusplus
}
#endif
#endif /* TESSPHOT_HIP_H */
