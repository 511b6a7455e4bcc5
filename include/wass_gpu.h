/*
 * wass_gpu.h -- C ABI of libwassgpu.so: the MI355X (gfx950) implementation of
 * the wass_stereo dense-stereo hot path.
 *
 * The reference has no in-process plugin API for this path; wass_stereo is one
 * process whose main() (src/wass_stereo/wass_stereo.cpp:1799-2149) calls
 * sgbm_dense_stereo / triangulate / PovMesh methods directly.  Each entry
 * point below replaces one of those reference interfaces (cited file:line,
 * relative to /root/reference/src) so that a maintainer can swap the body of
 * the corresponding function for one call.
 *
 * Conventions
 *   - every function returns 0 (WASS_OK) or a negative wass_status; nothing
 *     throws or aborts; wass_last_error(ctx) gives a message.
 *   - plain pointers and sizes only.  "_dev" variants take DEVICE pointers and
 *     are asynchronous on the context's stream; the others take HOST pointers
 *     and return when the result is in host memory.
 *   - a context owns one GPU, one stream and its scratch HBM.  One host thread
 *     per context; distinct contexts are independent (one per GPU / process).
 */
#ifndef WASS_GPU_H
#define WASS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    WASS_OK = 0,
    WASS_ERR_INVALID_ARG = -1,
    WASS_ERR_UNSUPPORTED = -2,   /* e.g. MAX_DISPARITY > 1024, WINSIZE > 17     */
    WASS_ERR_NO_MEMORY = -3,
    WASS_ERR_DEVICE = -4,        /* HIP runtime error, no GPU                  */
    WASS_ERR_COST_OVERFLOW = -5, /* int16 cost precondition violated (A.7)     */
    WASS_ERR_TOO_FEW_POINTS = -6
} wass_status;

typedef struct wass_ctx wass_ctx;

int wass_ctx_create(int device_id, wass_ctx** out);
/* Devices the HIP runtime of this process shows (0 without a usable GPU or runtime).  Lets a host tell "no GPU at all" (every entry
 * point fails loudly) from "this device index does not exist here" (another process, or device 0, can take the frame). */
int wass_device_count(int* n_devices);
void wass_ctx_destroy(wass_ctx* ctx);
const char* wass_last_error(const wass_ctx* ctx);
/* raw hipStream_t of the context (for callers that enqueue their own work) */
void* wass_ctx_stream(wass_ctx* ctx);
int wass_ctx_synchronize(wass_ctx* ctx);
/* The "_dev" entry points read caller-owned device buffers on the context's own (non-blocking) streams.  A caller
 * that produced those buffers on another stream calls this first: it orders all work enqueued on the context from now
 * on after everything already enqueued on producer_stream (a hipStream_t; NULL = the legacy default stream). */
int wass_ctx_wait_for_stream(wass_ctx* ctx, void* producer_stream);
/* Two-stage pipelining inside one context.  on != 0: every stage after the SGM call (wass_disparity_postprocess*,
 * wass_triangulate*, wass_mesh_*) is enqueued on a second stream that waits for the last wass_sgm_disparity_dev
 * call, so the tail of frame i (small, latency-bound kernels and the PCIe download) runs underneath the SGM stage
 * of frame i+1.  Reusing one disparity buffer for every frame is safe (the SGM call waits for the previous
 * frame's clean-up to have read it before its last kernel writes it); alternating two avoids that wait.
 * wass_ctx_synchronize waits for both streams. */
int wass_ctx_set_tail_overlap(wass_ctx* ctx, int on);
/* test mode: keep intermediates (the finished S volume) that production never writes to HBM */
int wass_ctx_set_debug(wass_ctx* ctx, int on);
const char* wass_version(void);

/* Asynchronous upload h_src -> d_dst on the context's copy stream (h_src: pinned host memory, valid until the copy has
 * executed).  The calls of this library that READ device inputs (wass_sgm_disparity_dev, wass_burned_area_mask_dev) wait
 * for the pending uploads that cover their input pointers, and everything later in a frame is ordered after the SGM
 * call; nothing else waits.  A driver that uploads frame i+1 just before it submits frame i (three input sets: the
 * buffer was last used by frame i-2) gets the transfer underneath frame i's kernels.  A kernel of the caller's own that
 * reads d_dst must be ordered by the caller (wass_ctx_synchronize, or pass the buffer through one of the calls above). */
int wass_upload_async(wass_ctx* ctx, void* d_dst, const void* h_src, size_t nbytes);
/* Device and pinned host memory for a host program that has no other GPU runtime of its own (the C++ sequence driver;
 * bench.py and the tests use torch's allocator instead): hipMalloc / hipHostMalloc on the context's device.  Device
 * memory comes back zero-filled.  Free with the matching call before the context is destroyed. */
int wass_device_alloc(wass_ctx* ctx, size_t nbytes, void** d_out);
void wass_device_free(wass_ctx* ctx, void* d_ptr);
/* d_src -> h_dst after everything enqueued on the context so far; returns when the bytes are in host memory */
int wass_download(wass_ctx* ctx, void* h_dst, const void* d_src, size_t nbytes);
/* cv::resize(src, dst, Size(dw, dh), 0, 0, INTER_CUBIC) of an 8-bit picture resident in HBM (the 0000000X_s.png previews of
 * load_data, wass_stereo.cpp:401-417): 11-bit fixed-point weights, the arithmetic of the DENSE_SCALE resampler.  On the context's
 * SGM stream; waits for pending uploads of d_src.  d_dst: dw * dh bytes, dense. */
int wass_resize_cubic_u8_dev(wass_ctx* ctx, const uint8_t* d_src, int sw, int sh, size_t src_stride, uint8_t* d_dst, int dw, int dh);
/* the same without waiting: the copy runs on the context's copy stream once everything enqueued so far on the SGM stream AND on
 * the tail stream (clean-up, triangulation, mesh stages under tail overlap) has finished; h_dst (pinned) is complete when a
 * later wass_ctx_frame_result() or wass_ctx_synchronize() returns */
int wass_download_async(wass_ctx* ctx, void* h_dst, const void* d_src, size_t nbytes);
int wass_pinned_alloc(wass_ctx* ctx, size_t nbytes, void** h_out);
void wass_pinned_free(wass_ctx* ctx, void* h_ptr);
/* DISCARD_BURNED_AREAS (wass_stereo.cpp:1072,1086): d_mask[i] = d_img[i] <= 254, on the context's SGM stream; feeds the
 * left_mask / right_mask arguments of wass_triangulate_dev.  Both pointers 4-byte aligned. */
int wass_burned_area_mask_dev(wass_ctx* ctx, const uint8_t* d_img, size_t n, uint8_t* d_mask);
/* The camera masks of triangulate() in general (wass_stereo.cpp:1057-1093): d_mask[i] = (d_file_mask ? d_file_mask[i] != 0 : 1)
 * && (d_img ? d_img[i] <= 254 : 1) -- LEFT_MASK_IMAGE / RIGHT_MASK_IMAGE thresholded by the caller (0/1 bytes), combined with
 * DISCARD_BURNED_AREAS on the device.  Either input may be NULL.  On the context's SGM stream; waits for pending uploads. */
int wass_camera_mask_dev(wass_ctx* ctx, const uint8_t* d_img, const uint8_t* d_file_mask, size_t n, uint8_t* d_mask);

/* ------------------------------------------------------------------------
 * cv::StereoSGBM parameters as sgbm_dense_stereo sets them
 * (wass_stereo/wass_stereo.cpp:742-759,772-782).
 *   ndirs = 5 : MODE_SGBM, what the reference runs (bit-exact parity mode)
 *   ndirs = 8 : MODE_HH  (the commented-out fullDP switch, :777)
 * ------------------------------------------------------------------------ */
typedef struct {
    int min_disp;         /* MIN_DISPARITY                                   */
    int num_disp;         /* MAX_DISPARITY, multiple of 16                   */
    int win;              /* WINSIZE (odd)                                   */
    int P1, P2;           /* DENSE_P1_MULT*win*win, DENSE_P2_MULT*win*win    */
    int uniq_ratio;       /* DENSE_UNIQUENESS_RATIO, at most 100 (< 0: 10)   */
    int disp12_max_diff;  /* DENSE_DISP12MAXDIFF                             */
    int prefilter_cap;    /* DENSE_PREFILTER_CAP                             */
    int speckle_win;      /* DENSE_SPECKLE_WINDOW_SIZE (> 0: cv::filterSpeckles) */
    int speckle_range;    /* DENSE_SPECKLE_RANGE                             */
    int ndirs;            /* 5 or 8                                          */
    int disp_offset;      /* DISPARITY_OFFSET (:747,801-812)                 */
    double dense_scale;   /* DENSE_SCALE (:745)                              */
} wass_sgm_params;

/* Replaces wass_stereo.cpp:820-839: zero-pad both rectified crops, run
 * dense_stereo->compute(right_image, left_image, disparity), crop columns
 * [num_disp, num_disp + w).  right/left: w x h u8, pitch in bytes.
 * disp16_out: w x h int16 (4 fractional bits), in the right image's frame.
 * Returns WASS_ERR_COST_OVERFLOW (result still written) if a block cost
 * exceeded the int16 range the reference's scalar and SIMD builds agree on.
 * uniq_ratio above 100 is refused with WASS_ERR_INVALID_ARG: the reference's
 * factor 100 - ratio is then negative and it rejects every pixel with a
 * positive cost outside best +- 1, which the selection kernels' unsigned
 * 24-bit product does not reproduce. */
/* DENSE_SCALE != 1 (:788-796): both crops are first resized with cv::resize INTER_CUBIC -- by (scale, 1) when the scale is
 * above 1, by (scale, scale) below -- and disp16_out has the size of the RESIZED crops: */
int wass_dense_input_size(int w, int h, double dense_scale, int* ws, int* hs);
int wass_sgm_disparity(wass_ctx* ctx, const uint8_t* right, const uint8_t* left,
                       int w, int h, size_t pitch, const wass_sgm_params* p,
                       int16_t* disp16_out);
int wass_sgm_disparity_dev(wass_ctx* ctx, const uint8_t* d_right, const uint8_t* d_left,
                           int w, int h, size_t pitch, const wass_sgm_params* p,
                           int16_t* d_disp16_out);

/* Stage timings of the last wass_sgm_disparity[_dev] call, measured with
 * hipEvents on the context's stream (milliseconds).  Synchronises. */
typedef struct {
    float prefilter_ms;   /* K1: Sobel/BT interval images                     */
    float cost_ms;        /* K2: block-summed cost volume C                   */
    float aggregate_ms;   /* K3: all path sweeps (the roofline kernel family) */
    float select_ms;      /* K4: WTA/uniqueness/subpixel/disp2/L-R            */
    float median_ms;      /* K5: median 3x3 + crop                            */
    float total_ms;
    int   aggregate_launches;
    int   cost_overflow;  /* 1 if the int16 precondition was violated         */
    float vsum_ms;        /* part of cost_ms: the vertical block sum, which also
                             runs path 2 (column checkpoints / S = L_2)       */
} wass_sgm_timings;
int wass_sgm_last_timings(wass_ctx* ctx, wass_sgm_timings* out);
/* the call before the last one: lets a pipelined driver read frame n's stage times after frame n+1 has been
 * enqueued, without waiting for frame n+1 */
int wass_sgm_prev_timings(wass_ctx* ctx, wass_sgm_timings* out);
/* number of wass_sgm_disparity[_dev] calls of this context that were enqueued completely (a failed call does not count): a
 * pipelined driver remembers the value after its frame's call and later picks last / prev timings by the difference */
int wass_sgm_call_count(wass_ctx* ctx, uint64_t* n_calls);
/* stage times of call number `call` (1-based, as counted by wass_sgm_call_count right after the call); the last four calls are kept */
int wass_sgm_call_timings(wass_ctx* ctx, uint64_t call, wass_sgm_timings* out);

/* Device-side canary for the aggregation kernels: runs one synthetic w x h pair with num_disp disparities through the
 * production schedule (checkpoint sweeps, pair kernels with recomputation, row fusion) and through one plain sweep per path,
 * and compares the two aggregated volumes S cell by cell ON THE DEVICE -- no CPU oracle, usable in the field.  *mismatches
 * receives the number of differing cells; returns WASS_ERR_DEVICE when it is not zero.  The two forms share the arithmetic
 * of one path step and nothing of the scheduling around it, which is where an instance-specific miscompile and a hardware
 * store hazard were found.  __graft_entry__.smoke() and tests/test_sgm_gpu.py run it for every NP. */
int wass_sgm_selftest(wass_ctx* ctx, int w, int h, int num_disp, int ndirs, uint64_t* mismatches);

/* Measurement hook for the roofline accounting (bench.py): re-runs the vertical block sum of the LAST call on its retained
 * horizontal sums, once as the plain sum (plain_ms) and once in the form the call used (production_ms; in 8-path mode it
 * also carries paths 2 / 6 and their checkpoints, in 5-path mode path 2 and S = L_2), best of three, hipEvents on the
 * context's stream.  production_ms - plain_ms is what the column paths add to the cost stage.  Synchronises. */
int wass_sgm_probe_vsum(wass_ctx* ctx, float* plain_ms, float* production_ms);

/* Measurement hook (bench.py, "kernel_ms"): with on != 0 every kernel launch of the cost stage and of the aggregation family is
 * bracketed by two hipEvents on the stream it is launched on (main or side).  wass_sgm_kernel_times then returns the LAST SGM call's
 * launches in launch order: their names, '\n'-separated, into names[names_cap], and their durations into ms[max_kernels]; *n_kernels
 * = how many.  Off by default (an event between two kernels is a marker packet on the queue); synchronises. */
int wass_ctx_set_kernel_events(wass_ctx* ctx, int on);
int wass_sgm_kernel_times(wass_ctx* ctx, char* names, size_t names_cap, float* ms, int max_kernels, int* n_kernels);

/* Test hooks: copy intermediates of the last wass_sgm_disparity call to host.
 * C/S are [h][width1][num_disp] int16 with width1 = w + max(disp_offset,0) -
 * min_disp (C without the +P2 bias); raw is the padded-width disparity before
 * the 3x3 median ([h][w + num_disp + max(disp_offset,0)]).  Any may be NULL.
 * S_out requires wass_ctx_set_debug(ctx, 1) before the disparity call. */
int wass_sgm_debug_fetch(wass_ctx* ctx, int16_t* C_out, int16_t* S_out, int16_t* raw_out);


/* ------------------------------------------------------------------------
 * Disparity clean-up, rows a7-a9.  Replaces wass_stereo.cpp:853-945 (this form:
 * DENSE_SCALE == 1, see _ex below): clean_and_convert_disparity (:714-733), DISP_DILATE_STEPS
 * x matrix_dilate_zero (:617-662, including its column-shift quirk),
 * DISP_EROSION_STEPS x matrix_erode_zero (:665-711), the same-size
 * NN/cubic resize + extra erosion mask (:903-928) and the optional
 * cv::medianBlur (:941-945; MEDIAN_FILTER_WSIZE 0, 3 or 5).
 * disp16: w x h int16 as produced by wass_sgm_disparity; out: w x h float32.
 * ------------------------------------------------------------------------ */
int wass_disparity_postprocess(wass_ctx* ctx, const int16_t* disp16, int w, int h,
                               const wass_sgm_params* p, int dilate_steps, int erode_steps,
                               int median_wsize, float* disp_f32_out);
int wass_disparity_postprocess_dev(wass_ctx* ctx, const int16_t* d_disp16, int w, int h,
                                   const wass_sgm_params* p, int dilate_steps, int erode_steps,
                                   int median_wsize, float* d_disp_f32_out);
/* The same with every option of wass_stereo.cpp:853-986: disp16 is ws x hs (wass_dense_input_size), the result is
 * out_w x out_h = roi_comb_right.size(): the converted map is multiplied by 1/DENSE_SCALE (:853), resized with
 * cv::resize INTER_NEAREST and INTER_CUBIC (:903-904), masked by the eroded nearest copy (:908-928), median-filtered,
 * and -- cc_threshold = DENSE_DISPARITY_BIGGEST_COMPONENT_THRESHOLD > 0 -- zeroed where the squared 3x3 Sobel gradient
 * exceeds the threshold and outside the largest 8-connected component of what is left (:947-986). */
int wass_disparity_postprocess_ex(wass_ctx* ctx, const int16_t* disp16, int ws, int hs, const wass_sgm_params* p,
                                  int dilate_steps, int erode_steps, int median_wsize, int cc_threshold,
                                  int out_w, int out_h, float* disp_f32_out);
int wass_disparity_postprocess_ex_dev(wass_ctx* ctx, const int16_t* d_disp16, int ws, int hs, const wass_sgm_params* p,
                                      int dilate_steps, int erode_steps, int median_wsize, int cc_threshold,
                                      int out_w, int out_h, float* d_disp_f32_out);
/* :947-986 alone, in place on a device map (test hook / building block) */
int wass_biggest_component_by_gradient_dev(wass_ctx* ctx, float* d_disp, int w, int h, int threshold);
/* the "large gradient" mask (non-zero where the squared Sobel magnitude exceeded the threshold, :951-957) of the last
 * component extraction on this context (cc_threshold > 0 in wass_disparity_postprocess_ex or the call above), w x h bytes to
 * the host: what the reference paints into disparity_large_gradient.jpg (:958-960) */
int wass_large_gradient_mask(wass_ctx* ctx, int w, int h, uint8_t* mask_out);
/* cv::filterSpeckles(img, new_val, max_size, max_diff) alone, in place on a device int16 map of w x h (the filter that
 * wass_sgm_disparity applies when speckle_win > 0; test hook / building block): 4-connected regions of pixels != new_val
 * whose neighbours differ by at most max_diff; a region of at most max_size pixels becomes new_val.  new_val is an int16
 * value, max_size and max_diff are >= 0.  Asynchronous on the stream of the clean-up calls. */
int wass_filter_speckles_dev(wass_ctx* ctx, int16_t* d_img, int w, int h, int new_val, int max_size, int max_diff);

/* ------------------------------------------------------------------------
 * Triangulation, rows a10-a13.  Replaces triangulate(StereoMatchEnv&)
 * (wass_stereo.cpp:1039-1386), StereoMatchEnv::unrectify (:299-324) and
 * triangulate(p,q,R,T) (wass_lib/triangulate.hpp:26-72).  All matrices are
 * row-major doubles.
 * ------------------------------------------------------------------------ */
typedef struct {
    double K_left[9], K_right[9];   /* env.intrinsics_left / _right                 */
    double R[9], T[3];              /* env.R, env.T (|T| = 1, :360-370)             */
    int    use_custom;              /* USE_CUSTOM_STEREORECTIFY                     */
    double R1[9], R2[9];            /* env.rec_R1 / rec_R2        (OpenCV path)     */
    double P1[12], P2[12];          /* env.rec_P1 / rec_P2 (3x4)  (OpenCV path)     */
    double HLi[9], HRi[9];          /* env.HLi / HRi              (custom path)     */
    double disparity_compensation;  /* env.disparity_compensation (:804-812)        */
    double dense_scale;             /* DENSE_SCALE                                  */
} wass_geom;

typedef struct {
    double min_angle_deg;           /* TRIANG_MIN_ANGLE                             */
    double bbox[4];                 /* left, top, right, bottom in the left image;
                                       defaults (0,0,cols,rows) (:1046-1054)        */
    double cam_distance;            /* env.cam_distance (= 1)                       */
} wass_tri_params;

/* organised point cloud on the device: PovMesh (wass_stereo/PovMesh.h:28-88) as
 * structure-of-arrays (valid u8, x/y/z f64, gray u8), index v*width+u */
typedef struct wass_mesh wass_mesh;

/* disp_roi: roi_r[2] x roi_r[3] float32, the part of env.disparity inside
 * roi_comb_right (the reference map is zero elsewhere).  W,H: size of the
 * rectified frames.  roi_* = {x, y, width, height}.  right_img: the undistorted
 * RIGHT image (env.right, img_w x img_h) sampled for the point grey value
 * (:1342).  left_mask/right_mask: 0/1 images of the originals' size or NULL
 * (= all ones) (:1057-1093).  Host pointers; *_dev takes device pointers.
 * n_pts may be NULL for the *_dev form: the point count is then not read back
 * and the call does not synchronise with the host. */
int wass_triangulate(wass_ctx* ctx, const float* disp_roi, int W, int H,
                     const int roi_l[4], const int roi_r[4], const wass_geom* g,
                     const uint8_t* right_img, int img_w, int img_h,
                     const uint8_t* left_mask, const uint8_t* right_mask,
                     const wass_tri_params* tp, wass_mesh** out, uint64_t* n_pts);
int wass_triangulate_dev(wass_ctx* ctx, const float* d_disp_roi, int W, int H,
                         const int roi_l[4], const int roi_r[4], const wass_geom* g,
                         const uint8_t* d_right_img, int img_w, int img_h,
                         const uint8_t* d_left_mask, const uint8_t* d_right_mask,
                         const wass_tri_params* tp, wass_mesh** out, uint64_t* n_pts);
/* ---- the debug pictures of a frame, rendered and JPEG-coded on the device (replaces the cv::imwrite calls of wass_stereo.cpp:833, 854,
 * 1001, 1017, 1381-1382, 1925 and PovMesh.cpp:982-984).  Baseline JPEG, quality 95 like cv::imwrite's default,
 * 4:4:4, a restart marker after every row of blocks; the same bytes as the host writer of wass_amd/host/jpeg.hpp gives for the same
 * pixels (shared integer arithmetic, csrc/jpeg_spec.h). */
enum {
    WASS_PIC_STEREO = 0,           /* stereo.jpg                   rectified pair side by side, ROI rectangles, a red line every 20 rows */
    WASS_PIC_STEREO_INPUT = 1,     /* stereo_input.jpg             the two zero-padded SGBM inputs, left above right */
    WASS_PIC_DISPARITY_RAW = 2,    /* disparity_stereo_ouput.jpg   render_disparity_float of the converted raw disparity */
    WASS_PIC_DISPARITY_FINAL = 3,  /* disparity_final_scaled.jpg   ... of the final map */
    WASS_PIC_COVERAGE = 4,         /* disparity_coverage.jpg       right picture, green where disparity > 1, half size */
    WASS_PIC_R0 = 5,               /* undistorted/R0.jpg           grey where a point was triangulated, else the rejecting test's colour */
    WASS_PIC_R1 = 6,               /* undistorted/R1.jpg           the same with the matched left pixel's grey */
    WASS_PIC_COMPONENTS = 7,       /* graph_components.jpg         biggest component green, the other points blue, half size */
    WASS_DEBUG_PICTURES = 8
};
typedef struct wass_debug_desc {
    int W0, H0;                        /* size of the full rectified pictures */
    int roi_l[4], roi_r[4];            /* x, y, width, height of the two crops (equal sizes) */
    const uint8_t* d_left_crop;        /* the rectified crops the SGM stage was given (dense, roi-sized, in HBM) */
    const uint8_t* d_right_crop;
    const int16_t* d_disp16;           /* wass_sgm_disparity_dev's output for them */
    const float* d_dispf;              /* wass_disparity_postprocess_dev's output */
    int num_disp, min_disp, disp_offset;
    double disparity_compensation;
    int quality;                       /* 0 = 95 */
} wass_debug_desc;
/* One picture that exists in HBM (grey: channels 1, or r,g,b interleaved: 3) as a complete JPEG file in h_dst; synchronous. */
int wass_jpeg_encode_dev(wass_ctx* ctx, const uint8_t* d_pixels, int w, int h, int channels, size_t pitch_bytes, int quality,
                         uint8_t* h_dst, size_t capacity, size_t* nbytes);
/* width, height and channels (1 grey, 3 colour) of picture k for this frame geometry: what a caller sizes its slots by */
int wass_debug_picture_size(const wass_debug_desc* desc, int k, int* width, int* height, int* channels);
/* All eight pictures of the frame whose mesh is `mesh`, enqueued behind the frame's tail (call it after wass_mesh_finish_frame_async*
 * with a component mask destination, before destroying the mesh).  h_dst: pinned host memory (wass_pinned_alloc); picture k is written
 * as a complete file at h_dst + offset[k] by the kernels themselves, offset[0] = 0, offset[k + 1] = offset[k] + capacity[k] rounded up
 * to a multiple of 64.  Nothing is synchronised: wass_debug_pictures_result(ticket) waits for this frame's pictures and gives their
 * sizes (0: the picture did not fit into its slot and was not written).  Four tickets may be outstanding. */
int wass_debug_pictures_async(wass_ctx* ctx, const wass_mesh* mesh, const wass_debug_desc* desc, uint8_t* h_dst,
                              const size_t capacity[WASS_DEBUG_PICTURES], uint64_t* ticket);
int wass_debug_pictures_result(wass_ctx* ctx, uint64_t ticket, size_t nbytes[WASS_DEBUG_PICTURES]);

/* Why triangulate kept or rejected each pixel of the grid: what the reference paints into its debug pictures
 * undistorted/R0.jpg (low nibble) and R1.jpg (high nibble), wass_stereo.cpp:1111-1119,1216-1338.  codes_out: width x
 * height bytes (host). */
enum {
    WASS_CODE_NONE = 0,            /* not processed (no disparity): black */
    WASS_CODE_GREY = 1,            /* triangulated: the rectified image's grey value */
    WASS_CODE_OUTSIDE_IMAGE = 2,   /* teal   (255,255,0) BGR */
    WASS_CODE_OUTSIDE_BBOX = 3,    /* yellow (0,255,255): outside the bounding box or masked out */
    WASS_CODE_ANGLE = 4,           /* green  (0,255,0): rays too parallel */
    WASS_CODE_TOO_CLOSE = 5,       /* blue   (255,0,0) */
    WASS_CODE_TOO_DISTANT = 6      /* red    (0,0,255) */
};
int wass_mesh_reject_codes(wass_ctx* ctx, const wass_mesh* m, uint8_t* codes_out);
void wass_mesh_destroy(wass_mesh* m);
int wass_mesh_size(const wass_mesh* m, int* width, int* height);
/* copy the cloud to host (test hook, PLY / xyzbin writers): valid[w*h],
 * p3d[w*h*3] (interleaved xyz), gray[w*h]; any may be NULL */
int wass_mesh_download(wass_ctx* ctx, const wass_mesh* m, uint8_t* valid, double* p3d, uint8_t* gray);
/* build a mesh from host arrays (test hook) */
int wass_mesh_upload(wass_ctx* ctx, int width, int height, const uint8_t* valid, const double* p3d,
                     const uint8_t* gray, wass_mesh** out);

/* ------------------------------------------------------------------------
 * PovMesh stages, rows a14-a20 (wass_stereo/PovMesh.cpp).
 * ------------------------------------------------------------------------ */
/* compute_zgap_percentile (:888-926); exact order statistic; NaN if no gaps (always so for width < 3 or height < 2).
 * Undefined for NaN heights: the reference sorts them. */
int wass_mesh_zgap_percentile(wass_ctx* ctx, wass_mesh* m, double percentile, double* out, uint64_t* n_gaps);
/* cluster_biggest_connected_component (:929-987): keep the largest 4-connected
 * component of valid points whose |dz| < zgap (first in column-major order on ties) */
int wass_mesh_keep_biggest_component(wass_ctx* ctx, wass_mesh* m, double zgap, uint64_t* size_out);
/* ransac_find_plane (:665-777).  uv_triplets[rounds][6] = {u1,v1,u2,v2,u3,v3}
 * drawn by the caller with rand() as in :680-691 (wass_ransac_sample does that).
 * Returns WASS_OK with *found = 0 when best < width*height/10 (:773).
 * rounds: 1 .. 1800, more is WASS_ERR_UNSUPPORTED (also in wass_mesh_fit_plane and wass_mesh_finish_frame_async*); a sample
 * outside the grid is WASS_ERR_INVALID_ARG.  A valid point with a NaN coordinate is never an inlier (fabs(NaN) < thr is false),
 * neither here nor in wass_mesh_crop_plane, which drops it; a triple that spans no plane (two samples on one pixel, collinear
 * points) gives a NaN candidate that counts 0. */
int wass_ransac_sample(int width, int height, int rounds, int32_t* uv_triplets);
/* The same draw from a PRIVATE generator that restates glibc's srand(seed) + rand(): what the reference gets for
 * RANDOM_SEED = seed (wass_stereo.cpp:1864-1872; RANSAC is its only rand() consumer), independent of whoever else in
 * the process calls rand() -- threads of the HIP runtime do. */
int wass_ransac_sample_seeded(uint32_t seed, int width, int height, int rounds, int32_t* uv_triplets);
int wass_mesh_ransac_plane(wass_ctx* ctx, wass_mesh* m, const int32_t* uv_triplets, int rounds,
                           double thr, double plane_out[4], uint64_t* best_inliers, int* found);
/* crop_plane (:780-815) */
int wass_mesh_crop_plane(wass_ctx* ctx, wass_mesh* m, const double plane[4], double thr, uint64_t* kept);
typedef struct {
    double xmin, xmax, ymin, ymax;  /* PLANE_REFINE_{XMIN,XMAX,YMIN,YMAX}           */
    double max_distance;            /* PLANE_REFINEMENT_MAX_DISTANCE                */
    int weight_by_distance;         /* PLANE_WEIGHT_PROPORTIONAL_TO_DISTANCE        */
    int central_third_only;         /* PLANE_USE_CENTRAL_THIRD_ONLY                 */
} wass_refine_params;
/* refine_plane (:581-660): weighted PCA plane through the inliers */
int wass_mesh_refine_plane(wass_ctx* ctx, wass_mesh* m, const wass_refine_params* rp,
                           double plane_out[4], uint64_t* n_inliers);
/* plane_refinement_inliers.xyz (wass_stereo.cpp:2077-2085): the points main() writes after refine_plane -- every
 * `every`-th (10) refinement inlier of PovMesh.cpp:590-606 in raster order -- selected on the device.  *xyz_out: malloc'ed
 * n_out x 3 doubles (release with wass_free); NULL when there is none. */
int wass_mesh_refinement_inliers(wass_ctx* ctx, wass_mesh* m, const wass_refine_params* rp, int every, double** xyz_out,
                                 uint64_t* n_out);
/* Fused forms of the calls above for throughput: same results, but every intermediate decision (radix-select
 * digits, winning component, best RANSAC candidate, centroid, 3x3 eigenvector) is taken on the device and the
 * host reads back once.
 *   wass_mesh_remove_outliers = zgap_percentile + keep_biggest_component   (wass_stereo.cpp:2046-2050)
 *   wass_mesh_fit_plane       = ransac_plane -> crop_plane(ransac_thr) -> refine_plane -> crop_plane(max_distance)
 *                               (wass_stereo.cpp:2062-2107); found == 0: nothing cropped, plane = NaN */
int wass_mesh_remove_outliers(wass_ctx* ctx, wass_mesh* m, double percentile, double* zgap_out, uint64_t* n_gaps,
                              uint64_t* size_out);
typedef struct {
    int      found;                 /* RANSAC succeeded (best >= width*height/10)   */
    double   ransac_plane[4];
    uint64_t ransac_inliers;
    double   plane[4];              /* refined plane                                 */
    uint64_t refine_inliers;
    uint64_t kept_after_ransac_crop, kept_final;
} wass_plane_result;
int wass_mesh_fit_plane(wass_ctx* ctx, wass_mesh* m, const int32_t* uv_triplets, int rounds, double ransac_thr,
                        const wass_refine_params* rp, double max_distance, wass_plane_result* out);
/* Everything main() does with the mesh after triangulation (wass_stereo.cpp:2046-2123: z-gap percentile, biggest
 * component, RANSAC plane, crop, refine, crop, mesh_cam.xyzC) enqueued WITHOUT a host synchronisation: all
 * decisions are taken on the device (RANSAC failure -> nothing cropped, identity R|T in the header, like
 * wass_mesh_encode_xyzc(plane = NULL)).  dst receives the file image (148-byte header + 6 bytes per point; it must
 * hold 148 + 6*width*height bytes, pinned memory recommended) through the context's copy stream.
 * wass_ctx_frame_result() waits for that download and reports what the stage-by-stage calls would have returned;
 * the number of valid bytes in dst is result.xyzc_bytes.  TWO frames may be pending per context (round 5): a driver enqueues
 * frame n+1's tail before it reads frame n's record, so that the tail stream goes from one frame's tail straight into the next
 * one's; wass_ctx_frame_result() hands the records out in submission order, a third wass_mesh_finish_frame_async* call without a
 * read in between is refused.  dst (and inliers_dst / inliers_text_dst) of a pending frame must stay untouched until its record
 * has been read. */
typedef struct {
    double   zgap;  uint64_t n_gaps, component_size;
    int      found, refine_ok;      /* refine_ok == 0 with found == 1: fewer than 3 refinement inliers (the
                                       stage-by-stage call returns WASS_ERR_TOO_FEW_POINTS)                     */
    double   ransac_plane[4];  uint64_t ransac_inliers;
    double   plane[4];         uint64_t refine_inliers, kept_after_ransac_crop, kept_final;
    uint64_t n_points, xyzc_bytes;
    /* status of the wass_sgm_disparity_dev call that produced the frame's disparity (the asynchronous SGM entry point
     * cannot return it): 1 = block cost + P2 left the int16 range where the reference is defined (the synchronous call
     * returns WASS_ERR_COST_OVERFLOW), -1 = unknown (the disparity did not come from this context's last two calls) */
    int      sgm_cost_overflow, sgm_timeout;
    /* valid points the last wass_triangulate[_dev] call of this context produced ("N valid points found",
     * wass_stereo.cpp:1374; the MIN_TRIANGULATED_POINTS test of :1993) -- counted on the device, no synchronisation */
    uint64_t n_triangulated;
    /* points written to inliers_dst by wass_mesh_finish_frame_async_ex (0 for the plain form or when RANSAC failed) */
    uint64_t n_inliers_out;
    /* GPU time (hipEvents on the context's tail stream, milliseconds) of the reference's timer rows after "Dense Stereo"
     * (wass_stereo.cpp:1982,2047,2049,2065,2089): [0] Triangulation, [1] Z-gap stats, [2] Outlier removal, [3] Plane fitting,
     * [4] Plane refinement (crop, refinement, crop, mesh_cam.xyzC image).  Zero when the mesh did not come from a
     * wass_triangulate[_dev] call of this context.  Under tail overlap the tail shares the GPU with the next frame's SGM stage. */
    float stage_ms[5];
    int reserved;
    /* wass_mesh_finish_frame_async_ex2: bytes of plane_refinement_inliers.xyz text in inliers_text_dst, and how many of its numbers
     * the device formatter could not write (inf, nan, |v| >= 1e6 or < 1e-22; never a triangulated coordinate): when that is not
     * zero the text is NOT the file -- format inliers_dst on the host instead */
    uint64_t inliers_text_bytes;
    uint32_t inliers_text_unsupported, reserved2;
} wass_frame_result;
int wass_mesh_finish_frame_async(wass_ctx* ctx, wass_mesh* m, double percentile, const int32_t* uv_triplets, int rounds,
                                 double ransac_thr, const wass_refine_params* rp, double max_distance, void* dst,
                                 size_t capacity);
/* The same, and additionally what main() writes to plane_refinement_inliers.xyz (wass_stereo.cpp:2077-2085): every
 * `inliers_every`-th refinement inlier (PovMesh.cpp:590-606) in raster order, selected on the device between the
 * refinement and the final crop and downloaded next to the file image -- inliers_dst: pinned host memory for
 * inliers_capacity points of 3 doubles (ceil(width*height / inliers_every) is always enough); NULL: not wanted.
 * component_mask_dst: pinned host memory for width*height bytes, the validity mask as cluster_biggest_connected_component leaves
 * it (PovMesh.cpp:929-987) -- before the plane stages crop it further; what graph_components.jpg is drawn from; NULL: not wanted. */
int wass_mesh_finish_frame_async_ex(wass_ctx* ctx, wass_mesh* m, double percentile, const int32_t* uv_triplets, int rounds,
                                    double ransac_thr, const wass_refine_params* rp, double max_distance, void* dst,
                                    size_t capacity, double* inliers_dst, size_t inliers_capacity, int inliers_every,
                                    uint8_t* component_mask_dst);
/* The same, and the file's TEXT as well: "x y z\n" per selected inlier, every number as a default-constructed std::ofstream
 * prints a double (precision 6, %g -- wass_stereo.cpp:2077-2085), formatted ON THE DEVICE (csrc/fmt_g6.h: correctly rounded in
 * 128-bit integer arithmetic, the characters of printf("%g")).  1.4 million numbers per 5-megapixel frame are a third of a
 * worker's host time when the host formats them.  inliers_text_dst: pinned host memory for 40 * ceil(width*height /
 * inliers_every) bytes (a line is at most 39 bytes); the valid length comes back in wass_frame_result.inliers_text_bytes.  When
 * the buffer is pinned host memory (wass_pinned_alloc, hipHostMalloc) the kernel writes the text straight into it and exactly the
 * file's bytes cross PCIe.  inliers_dst may be NULL then (the points are not downloaded); should inliers_text_unsupported come
 * back non-zero, wass_ctx_frame_inliers() fetches them for the host's formatter -- before the next frame's tail is enqueued. */
int wass_mesh_finish_frame_async_ex2(wass_ctx* ctx, wass_mesh* m, double percentile, const int32_t* uv_triplets, int rounds,
                                     double ransac_thr, const wass_refine_params* rp, double max_distance, void* dst,
                                     size_t capacity, double* inliers_dst, size_t inliers_capacity, int inliers_every,
                                     uint8_t* component_mask_dst, char* inliers_text_dst, size_t inliers_text_capacity);
/* one number as the device writes it (the same code built for the host): the characters of printf("%g", v) in out[0 .. return),
 * or -1 outside the formatter's domain.  out must hold 16 bytes.  Pure host function: no context, no GPU. */
int wass_format_g6(double v, char* out);
/* the selected inlier points of the frame whose wass_ctx_frame_result() was read last (n_inliers_out of them), copied on demand and
 * synchronously; valid until the next wass_mesh_finish_frame_async* call of the context */
int wass_ctx_frame_inliers(wass_ctx* ctx, double* dst, size_t capacity_points, uint64_t* n_out);
int wass_ctx_frame_result(wass_ctx* ctx, wass_frame_result* out);

/* RT_from_plane (:1044-1069); pure host math */
void wass_RT_from_plane(const double plane[4], double R[9], double T[3], double Rinv[9], double Tinv[3]);
/* save_as_xyz_compressed (:377-460): returns the exact bytes of mesh_cam.xyzC
 * in a malloc'ed host buffer (free with wass_free).  plane == NULL (RANSAC
 * failed): identity R, zero T are used (the reference reads uninitialised
 * memory there; documented divergence). */
int wass_mesh_encode_xyzc(wass_ctx* ctx, wass_mesh* m, const double plane[4], void** bytes, size_t* nbytes);
/* same, into a caller-owned buffer (>= 148 + 6*width*height bytes is always enough; pinned memory avoids a
 * staging copy) */
int wass_mesh_encode_xyzc_to(wass_ctx* ctx, wass_mesh* m, const double plane[4], void* dst, size_t capacity,
                             size_t* nbytes);
/* same, but returns as soon as the size is known: the 148-byte header is complete, the 6*n payload bytes are
 * being written by a DMA engine on the context's copy stream and are complete after wass_ctx_synchronize().
 * dst should be pinned host memory.  Lets a sequence driver overlap the PCIe transfer (and the file write of
 * wass_stereo.cpp:2123) with the next frame. */
int wass_mesh_encode_xyzc_async(wass_ctx* ctx, wass_mesh* m, const double plane[4], void* dst, size_t capacity,
                                size_t* nbytes);
void wass_free(void* p);

/* ---- row f3: the first step of the gridding stage from the device-resident mesh ----------------------------------
 * gridding/wassgridsurface/wassgridsurface.py:316-365 (_grid_task, "IDW"): align the cloud on the sequence's mean sea
 * plane (R, T = wass_RT_from_plane(mean plane), z negated: wass_utils.py:38-61), scale by the baseline in metres, bin the
 * points on the width x height grid over [xmin,xmax] x [ymin,ymax] (:322-326) and fill the gaps with
 * IDWInterpolator(KSIZE=5, exp=2.4, reps=1) (IDWInterpolator.py:23-58).  grid_out: height x width float32, NaN outside
 * the closed point mask; mask_out (may be NULL) that mask.  A cell takes the mean of its points (deterministic) where the
 * reference takes the median of ten random sub-samples (randomised): see grid.hip.
 * A point's column is floor((x - xmin) / (xmax - xmin) * (width - 1) + 0.5) in fp64, with the reference's order of roundings
 * (no precomputed scale), its row likewise; a point whose column or row falls outside the grid, or whose aligned x or y is
 * NaN or infinite, is dropped. */
typedef struct {
    double R[9], T[3];              /* gridsetup["Rpl"], ["Tpl"]                        */
    double baseline;                /* gridsetup["CAM_BASELINE"] (metres)               */
    double xmin, xmax, ymin, ymax;  /* grid extent in metres                            */
    int    width, height;           /* XX.shape[1], XX.shape[0]                         */
} wass_grid_setup;
int wass_mesh_grid_idw(wass_ctx* ctx, const wass_mesh* m, const wass_grid_setup* gs, float* grid_out, uint8_t* mask_out);
/* The same with the cell statistic chosen: WASS_GRID_CELL_MEAN (what wass_mesh_grid_idw computes) or WASS_GRID_CELL_MEDIAN, the
 * exact median of the points of a cell -- deterministic, independent of the point order, and robust against a few outliers
 * in a cell like the reference's nanmedian of random sub-samples (:330-345), whose expected value it is. */
enum { WASS_GRID_CELL_MEAN = 0, WASS_GRID_CELL_MEDIAN = 1 };
int wass_mesh_grid_idw_ex(wass_ctx* ctx, const wass_mesh* m, const wass_grid_setup* gs, int cell_statistic, float* grid_out,
                          uint8_t* mask_out);

/* ---- row f3, the reference's default interpolator: DCT surface interpolation -----------------------------------------
 * gridding/wassgridsurface/DCTInterpolator.py (wassgridsurface --ia DCT, the default: wassgridsurface.py:639): the cell map I
 * (NaN = no data) is fitted by the first nfreqs x nfreqs coefficients x of an orthonormal DCT-III basis, Irec = A_y^T x A_x,
 * minimising sum M (Irec - I)^2 / sum M + regularizer_alpha |x|_1 with torch.optim.Rprop (etas 0.5 / 1.2, step sizes
 * 1e-6 / 50) for max_iters + 1 steps; every 50th step stops when max |x_i - x_(i-1)| < tolerance_change.  grid_out
 * (height x width float32) is Irec of the final x, NaN where user_mask (height x width bytes, may be NULL) is 0
 * (wassgridsurface.py:355-357).  Extension: a rectangular grid uses a basis of size height for the rows and one of size
 * width for the columns (the reference raises a shape error unless width == height, where both agree).
 * x0 (nfreqs x nfreqs, may be NULL): the start value, e.g. the coeffs_out of the previous frame; NULL draws a deterministic
 * uniform [0, 1) one from opts->seed (the reference's torch.rand stream is not reproduced).  coeffs_out (nfreqs^2, may be
 * NULL): the final x.  Returns WASS_ERR_INVALID_ARG for nfreqs outside [1, min(width, height)] and WASS_ERR_TOO_FEW_POINTS
 * (grid_out all NaN) for a map without data.  The same inputs give the same bits on every run.  The solve runs on the
 * context's stream and the call returns when it has finished (the host checks the tolerance once per 50 steps). */
typedef struct {
    int    nfreqs;                  /* Nfreqs             (150)   */
    int    max_iters;               /* MAX_ITERS          (500)   */
    double tolerance_change;        /* TOLERANCE_CHANGE   (1e-4)  */
    double regularizer_alpha;       /* REGULARIZER_ALPHA  (8e-7)  */
    double learning_rate;           /* LEARNING_RATE      (5.0)   */
    uint64_t seed;                  /* start value when x0 is NULL (0) */
} wass_dct_opts;
typedef struct {
    int    steps;                   /* Rprop steps run                                   */
    int    converged;               /* 1: stopped by tolerance_change                    */
    double data_loss;               /* sum M (Irec - I)^2 / sum M of the final x         */
    double reg_loss;                /* |x|_1 of the final x                              */
    double fdelta;                  /* max |x_i - x_(i-1)| at the last check             */
} wass_dct_info;
void wass_dct_opts_default(wass_dct_opts* opts);
int wass_grid_dct(wass_ctx* ctx, const float* zz, int width, int height, const wass_dct_opts* opts, const float* x0,
                  const uint8_t* user_mask, float* grid_out, float* coeffs_out, wass_dct_info* info);
/* the same on device pointers (zz, x0, user_mask, grid_out, coeffs_out) */
int wass_grid_dct_dev(wass_ctx* ctx, const float* zz, int width, int height, const wass_dct_opts* opts, const float* x0,
                      const uint8_t* user_mask, float* grid_out, float* coeffs_out, wass_dct_info* info);
/* From the resident mesh: the alignment and binning of wass_mesh_grid_idw_ex (cell_statistic), then the solve above, with no
 * trip through the host.  cells_out (height x width float32, may be NULL): the binned cell map it solved on, NaN = empty
 * cell (the reference's ZZ). */
int wass_mesh_grid_dct(wass_ctx* ctx, const wass_mesh* m, const wass_grid_setup* gs, int cell_statistic, const wass_dct_opts* opts,
                       const float* x0, const uint8_t* user_mask, float* grid_out, float* cells_out, float* coeffs_out,
                       wass_dct_info* info);
/* One evaluation at x (nfreqs^2, host pointers): grad_out = the gradient of the loss above (alpha sign(x) included,
 * sign(0) = 0), data_loss and reg_loss = |x|_1 (either may be NULL).  For tests and for callers with their own optimiser. */
int wass_grid_dct_eval(wass_ctx* ctx, const float* zz, int width, int height, int nfreqs, double alpha, const float* x,
                       float* grad_out, double* data_loss, double* reg_loss);

/* ---- row f3, the sequence layer: what wassgridsurface --action grid does with the frames of a sequence -----------------
 * gridding/wassgridsurface/wassgridsurface.py:235-591 (grid): every frame binned, interpolated, masked, optionally median
 * filtered (--mf), pushed as millimetres into a count x Y x X cube, with the sequence's zmin / zmax / zmean, the per-point
 * average elevation and, with -z / --force-zero-mean, that average subtracted from every surface. */
/* Several cell maps of one shape in one DCT solve.  zz, grid_out: n_frames x height x width float32, contiguous; x0,
 * coeffs_out: n_frames x nfreqs x nfreqs or NULL (NULL x0: every frame starts from the seeded draw of opts->seed, as
 * wass_grid_dct does for each of them); user_mask: ONE height x width byte map for all frames, or NULL; info (may be NULL) and
 * status: n_frames entries.  Frame i is bit for bit what wass_grid_dct returns for zz[i], x0[i] and the same options: grid,
 * coefficients, steps, converged, data_loss, reg_loss, fdelta (the frames share launches, never a sum).  The stopping rule is
 * per frame: a frame below tolerance_change at a check step is finished and is not stepped again while the others go on.  A
 * frame without data gets an all-NaN grid, status[i] = WASS_ERR_TOO_FEW_POINTS and a zeroed info[i] (its coeffs_out are not
 * written) and does not disturb the others; status[i] = WASS_OK otherwise, and the call returns WASS_OK when the batch ran.
 * n_frames < 1 and the argument errors of wass_grid_dct return WASS_ERR_INVALID_ARG.  A large n_frames is walked in sub-batches
 * (scratch below 1 GiB); results do not depend on that. */
int wass_grid_dct_batch(wass_ctx* ctx, const float* zz, int n_frames, int width, int height, const wass_dct_opts* opts,
                        const float* x0, const uint8_t* user_mask, float* grid_out, float* coeffs_out, wass_dct_info* info,
                        int* status);
/* the same on device pointers (zz, x0, user_mask, grid_out, coeffs_out); info and status are host memory */
int wass_grid_dct_batch_dev(wass_ctx* ctx, const float* zz, int n_frames, int width, int height, const wass_dct_opts* opts,
                            const float* x0, const uint8_t* user_mask, float* grid_out, float* coeffs_out, wass_dct_info* info,
                            int* status);
/* The alignment and binning of wass_mesh_grid_idw_ex / wass_mesh_grid_dct alone (:316-346): the height x width float32 cell map
 * (NaN = empty cell, the reference's ZZ) into device memory, e.g. one slice of a batch buffer.  Enqueued on the context's
 * stream; the mesh must stay alive until that work has run (any synchronising call, such as the solve, will do). */
int wass_mesh_grid_cells_dev(wass_ctx* ctx, const wass_mesh* m, const wass_grid_setup* gs, int cell_statistic, float* d_cells);
/* --mf (:359-363): Zi[mask == 0] = 0; cv.medianBlur(Zi, ksize); Zi[mask == 0] = NaN on float32, n_frames maps at once, d_mask
 * (height x width bytes, shared, may be NULL) the final mask.  The border is replicated as cv::medianBlur does.  ksize 3 or 5
 * (cv::medianBlur takes no other size for 32-bit float, so the reference cannot either: WASS_ERR_INVALID_ARG); 0 only applies
 * the mask.  The median of an odd window is one of its elements: the result equals numpy's median over the edge-padded windows
 * bit for bit (a window that holds a NaN gives NaN).  d_in == d_out is refused.  Asynchronous on the context's stream. */
int wass_grid_median_dev(wass_ctx* ctx, const float* d_in, float* d_out, int n_frames, int width, int height, int ksize,
                         const uint8_t* d_mask);
/* What grid() keeps across the frames (:298-302, 490-494, 528-551, 554-576).
 * push (frames in sequence order, d_zi: n_frames x height x width metres on the device): per frame nanmean / nanmin / nanmax;
 * the per-point sum acc += (double)Zi in push order (NaN propagates, as Zmean_grids + Zi does); d_z_mm_out (may be NULL) =
 * Zi * 1000.0f, the float32 millimetres push_Z stores.  No floating-point atomics and a summation order that depends on the
 * grid size only: any split of the frames over the calls gives the same bits.
 * finish: zmin / zmax / zmean = np.amin / np.amax / np.mean of the per-frame values (one all-NaN frame makes them NaN);
 * mean_perpoint_mm (host, height x width, may be NULL) = acc / n_frames * 1000; with force_zero_mean zmean = 0 and
 * zmax = -zmin (:543-546).  frame_mean / frame_min / frame_max (host, one per pushed frame, may be NULL).
 * zero_mean (after finish): z = (float)((double)z - mean_perpoint_mm) on n_frames device maps of millimetres, the arithmetic of
 * the reference's chunked pass over the cube. */
typedef struct wass_grid_seq wass_grid_seq;
typedef struct {
    double zmin, zmax, zmean;       /* metres, like the reference's attributes          */
    int    n_frames;                /* frames pushed                                    */
} wass_grid_seq_stats;
int wass_grid_seq_create(wass_ctx* ctx, int width, int height, wass_grid_seq** out);
int wass_grid_seq_push_dev(wass_grid_seq* seq, const float* d_zi, int n_frames, float* d_z_mm_out);
int wass_grid_seq_finish(wass_grid_seq* seq, int force_zero_mean, wass_grid_seq_stats* stats, double* mean_perpoint_mm,
                         double* frame_mean, double* frame_min, double* frame_max);
int wass_grid_seq_zero_mean_dev(wass_grid_seq* seq, float* d_z_mm, int n_frames);
void wass_grid_seq_destroy(wass_grid_seq* seq);

/* ---- row f3, --ia LinearND (wassgridsurface.py:437-482): Delaunay linear interpolation of the cloud (grid_linear.hip) --------
 * The cloud (x_i, y_i, z_i), fp64, at the nodes of XX, YY = meshgrid(linspace(xmin, xmax, width), linspace(ymin, ymax, height)),
 * the nodes computed as numpy computes linspace.  Points taken: xmin <= x <= xmax and ymin <= y <= ymax, closed (the reference's
 * area_mask); a NaN or infinite coordinate drops the point; of several points with exactly the same (x, y) the lowest index
 * stands.  out: height x width fp64; flags: height x width bytes:
 *   0  the node lies in a triangle of three cloud points whose circumcircle holds no other point, both decided by fp64 orient and
 *      incircle determinants beyond their rounding bounds (DESIGN.md "LinearND"); with the vertices by index i < j < k the value is
 *      ((o_i z_i + o_j z_j) + o_k z_k) / ((o_i + o_j) + o_k), o_i = orient(P_j, P_k, q), o_j and o_k cyclically
 *   1  the node is beyond an edge of the cloud's convex hull by more than the bound: NaN, scipy's fill_value
 *   2  a triangle or a hull decision was found but not certified (cocircular points, collinear hull points, a node on a hull edge
 *      within the bound): the value of the triangle found, or NaN
 *   3  the walk reached its step cap (256): NaN
 * counts[4] (may be NULL): nodes per flag.  Fewer than three points taken, or all of them collinear: every value NaN, every
 * flag 1, WASS_ERR_TOO_FEW_POINTS.  WASS_ERR_INVALID_ARG: width or height < 1, xmax <= xmin with width > 1 (ymax, height likewise),
 * null pointers.  Only xmin .. height of gs are read by the array entries; the mesh entry aligns the resident mesh first, as
 * wass_mesh_grid_idw does (R, T, z negated, times the baseline).  Every entry runs on the context's stream, takes its scratch
 * from the context (wass_grid_linear_scratch_bytes says how much for n points, without a GPU) and returns after the stream has
 * run; the same input gives the same bits, in any order of the points once the indices are mapped. */
typedef struct {
    int max_walk_steps;             /* 0: 256                                                       */
    int accel_w, accel_h;           /* cells of the acceleration grid, 0: about sqrt(n / 2) a side  */
    int timing;                     /* != 0: fill ms_* of the info (three more events)              */
} wass_linear_opts;
typedef struct {
    uint64_t counts[4];             /* nodes per flag                                               */
    uint64_t n_taken;               /* points in the area, duplicates counted once                  */
    int hull_vertices;              /* of the convex hull handed to the walk                        */
    int hull_candidates;            /* points the device could not discard as interior              */
    int accel_w, accel_h;
    float ms_bucket, ms_hull, ms_walk;
} wass_linear_info;
int wass_grid_linear_dev(wass_ctx* ctx, const double* d_x, const double* d_y, const double* d_z, size_t n, const wass_grid_setup* gs,
                         double* d_out_f64, uint8_t* d_flags, uint64_t* counts);
int wass_grid_linear(wass_ctx* ctx, const double* x, const double* y, const double* z, size_t n, const wass_grid_setup* gs,
                     double* out_f64, uint8_t* flags, uint64_t* counts);
int wass_mesh_grid_linear(wass_ctx* ctx, const wass_mesh* mesh, const wass_grid_setup* gs, double* d_out_f64, uint8_t* d_flags,
                          uint64_t* counts);
int wass_grid_linear_scratch_bytes(size_t n, int width, int height, size_t* bytes);
/* The device entries with the full record (info may be NULL) and options (opts may be NULL).  The record is what
 * grid_sequence's linear_info needs beyond counts[4] (the points taken); the options are there for the tests (the step cap, the
 * pitch of the acceleration grid) and for scripts/time_linear_nd.py (timing), and no caller should depend on them: with accel_w or
 * accel_h set the call takes its scratch for THAT grid (cnt, off, fill: 12 bytes per cell), which
 * wass_grid_linear_scratch_bytes, stating the default grid, does not count. */
int wass_grid_linear_dev_ex(wass_ctx* ctx, const double* d_x, const double* d_y, const double* d_z, size_t n, const wass_grid_setup* gs,
                            const wass_linear_opts* opts, double* d_out_f64, uint8_t* d_flags, wass_linear_info* info);
int wass_mesh_grid_linear_ex(wass_ctx* ctx, const wass_mesh* mesh, const wass_grid_setup* gs, const wass_linear_opts* opts,
                             double* d_out_f64, uint8_t* d_flags, wass_linear_info* info);

/* Grid set-up (wassgridsurface.py:57-231, `--action setup`): the one step with real work in it, np.quantile over the heights of
 * the first frame's aligned cloud (:122-123), as exact order statistics on the device (grid_setup.hip).
 * wass_quantiles_f64_dev: out[i] = np.quantile(values, q[i]) (method "linear") over n doubles of device memory, i < nq, 1 <= nq <= 8,
 * every q[i] in [0, 1] (else WASS_ERR_INVALID_ARG).  Each double becomes an order-preserving 64-bit key; an MSD radix select in
 * 11-bit digits finds the order statistic a[lo] of every q in the same six passes, a[hi] is a[lo] where ties reach past lo and
 * the smallest key above a[lo] otherwise (one more pass); every decision stays on the device.  numpy's virtual index
 * (n - 1) * q and its _lerp (with the t >= 0.5 branch) are restated in fp64 on the host from those 2 nq values.  -0.0 sorts below
 * +0.0 (numpy leaves their order open; the values agree).  One NaN among the values makes every out[i] NaN, as np.quantile does.
 * n == 0: every out[i] is NaN and the call returns WASS_OK.
 * wass_mesh_aligned_z_quantiles: the same over the valid points of a mesh, of
 *     z = -(((R[6] x + R[7] y) + R[8] zc) + T[2]) * baseline
 * in fp64, every product and sum rounded on its own (no FMA): the third row of align_on_sea_plane_RT (wass_utils.py:54-61)
 * times the baseline.  R: 9 row-major doubles, T: 3.  n_points (may be NULL) receives the number of valid points; a mesh without
 * one gives NaN and WASS_OK.  The coordinates of invalid points are never read into the result.
 * Both return after a synchronisation.  wass_quantiles_launch_shape: the elements one workgroup takes per sweep and the elements
 * one launch takes per sweep (longer arrays are walked in several sweeps by the same launch), for tests that want those edges. */
int wass_quantiles_f64_dev(wass_ctx* ctx, const double* d_values, size_t n, const double* q, int nq, double* out);
int wass_mesh_aligned_z_quantiles(wass_ctx* ctx, const wass_mesh* m, const double R[9], const double T[3], double baseline,
                                  const double* q, int nq, double* out, uint64_t* n_points);
void wass_quantiles_launch_shape(int* per_block, int* per_launch);

/* ---- wave spectra of the gridded cube: postproc/wasspost/spectra.py as array functions ----------
 * compute_3D_spectrum (:53-171): Welch's method over 3-D segments of nt x ny x nx cells.  The host computes axes, windows
 * and the scale (wass_amd/postproc.py); one segment per push:
 *   fill     a NaN becomes its cell's mean over the segment's frames that are not NaN (np.nanmean(axis=0) of the float32
 *            segment times datascale); a cell that is NaN throughout is recorded in a device flag and enters as 0
 *   centre   minus the mean of the filled segment; times win_y[y] * win_x[x] * win_t[t] (fp64, then f32)
 *   DFT      along x (real to complex, kx = 0 .. nx / 2), y and t as products with f32 twiddle matrices on the f32 MFMA, every
 *            sum in a fixed order: the same segment gives the same bits on every run
 *   power    S[fftshift on the three axes] += |X|^2 in fp64, in push order; the half not computed is read at the mirrored
 *            (-f, -ky, -kx)
 * create: win_* are nt / ny / nx doubles (NULL: the symmetric Hann window of scipy.signal.windows.hann).  The handle owns
 * about six f32 copies of the window in device memory (wass_spec3d_scratch_bytes says how much: 1.1 GB at 100 x 684 x 684);
 * WASS_ERR_NO_MEMORY when that is more than 16 GiB or the allocation fails, WASS_ERR_INVALID_ARG for an axis outside
 * 1 .. 8192.
 * push: seg points at the segment's first cell, cell (t, y, x) at seg[t * stride_t + y * stride_y + x] (strides in
 * elements); host memory for wass_spec3d_push, device memory for wass_spec3d_push_dev (read in place).  Enqueued on the
 * context's stream; the host form returns when the segment has been handed to the runtime.
 * finish: S (host, nt x ny x nx doubles) = scale * the sum; *n_segments = segments pushed; *had_all_nan_cell = 1 if a cell
 * of some segment was NaN throughout (the reference's result is NaN everywhere then).  The handle starts over. */
typedef struct wass_spec3d wass_spec3d;
int wass_spec3d_scratch_bytes(int nt, int ny, int nx, size_t* bytes);
int wass_spec3d_create(wass_ctx* ctx, int nt, int ny, int nx, const double* win_t, const double* win_y, const double* win_x,
                       wass_spec3d** out);
int wass_spec3d_push(wass_spec3d* h, const float* seg, size_t stride_t, size_t stride_y, double datascale);
int wass_spec3d_push_dev(wass_spec3d* h, const float* d_seg, size_t stride_t, size_t stride_y, double datascale);
int wass_spec3d_finish(wass_spec3d* h, double scale, double* S, int* n_segments, int* had_all_nan_cell);
/* wass_spec3d_finish with S written to device memory (nt x ny x nx fp64, dense): the same bits, no download */
int wass_spec3d_finish_dev(wass_spec3d* h, double scale, double* d_S, int* n_segments, int* had_all_nan_cell);
void wass_spec3d_destroy(wass_spec3d* h);
/* compute_spectrum (:9-49): S[nperseg / 2 + 1] (host) = the sum over n_series series (host, n_series x n_samples float32) of
 * scipy.signal.csd(x, x, fs, nperseg=nperseg) with x = (float32)(series * scale) minus its mean: segments of nperseg with
 * overlap nperseg / 2, each minus its own mean, periodic Hann window, one-sided density scaling, mean over the segments.
 * nperseg > n_samples shrinks to n_samples (and the overlap with it), as csd does.  The DFT is the product of the 3-D
 * spectrum's x stage; sums in fp64 and in a fixed order. */
int wass_spec1d_welch(wass_ctx* ctx, const float* series, int n_series, int n_samples, int nperseg, double fs, double scale,
                      double* S);

/* ---- Butterworth filters of the gridded cube: wasspost filter / filter_fast (wasspost.py:149-314) and spatial_lowpass
 * (:318-371) as array functions.  The host designs the filters (wass_amd/postproc.py: butter_sos, sosfilt_zi).
 * wass_sosfiltfilt: scipy.signal.sosfiltfilt(sos, x, axis=0) with scipy's defaults for every cell of a count x H x W float32
 * cube, cell (t, y, x) at in[t * stride_t + y * stride_y + x] (strides in elements), the result as float32 at out with its own
 * strides (out may be in).  sos is n_sections x 6 doubles (b0 b1 b2 1 a1 a2, 1 .. 6 sections), zi n_sections x 2 doubles
 * (sosfilt_zi), padlen scipy's default for these sections (count > padlen, else WASS_ERR_INVALID_ARG).  The odd padding is
 * built in float32 as scipy builds it; both passes run in fp64 in scipy's order of operations and hand over in fp64;
 * remove_mean != 0 subtracts every series' fp64 time mean (summed first frame to last) before the cast.  A series that holds
 * a NaN comes out NaN throughout, no other is touched.  Rows are filtered in slabs of at most slab_rows (0: as many as fit
 * 16 GiB of scratch: (count + 2 padlen) * rows * W * 8 bytes, plus count * rows * W * 4 for the host form);
 * wass_sosfiltfilt_scratch_bytes says how much and how many rows, without a GPU.  The result does not depend on the slab
 * height and is the same bits on every run.  The host form returns with out filled; the device form enqueues on the
 * context's stream and frees its scratch after a synchronisation. */
int wass_sosfiltfilt_scratch_bytes(int count, int H, int W, int padlen, int slab_rows, int host, size_t* bytes, int* rows_per_slab);
int wass_sosfiltfilt(wass_ctx* ctx, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* sos,
                     int n_sections, const double* zi, int padlen, int remove_mean, int slab_rows, float* out, size_t out_stride_t,
                     size_t out_stride_y);
int wass_sosfiltfilt_dev(wass_ctx* ctx, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W,
                         const double* sos, int n_sections, const double* zi, int padlen, int remove_mean, int slab_rows,
                         float* d_out, size_t out_stride_t, size_t out_stride_y);
/* Spatial2DButterworth (spectra.py:176-202): out = real(ifft2(fft2(frame) * H)) per rows x cols float32 frame, H the UN-shifted
 * transfer function (rows x cols doubles, real and even: np.fft.ifftshift of the reference's array).  The transforms are the
 * DFT stages of the spectrum on the f32 MFMA, `batch` frames per launch (halved until the scratch fits 16 GiB;
 * wass_spatial_filter_scratch_bytes says how much).  A frame that holds a NaN comes out all NaN, no other is touched.  apply:
 * host frames, returns with out filled; apply_dev: device frames, enqueued on the context's stream (out may be the input). */
typedef struct wass_spatial_filter wass_spatial_filter;
int wass_spatial_filter_scratch_bytes(int rows, int cols, int batch, size_t* bytes);
int wass_spatial_filter_create(wass_ctx* ctx, int rows, int cols, const double* H, int batch, wass_spatial_filter** out);
int wass_spatial_filter_apply(wass_spatial_filter* h, const float* frames, size_t stride_t, size_t stride_y, int n_frames,
                              float* out, size_t out_stride_t, size_t out_stride_y);
int wass_spatial_filter_apply_dev(wass_spatial_filter* h, const float* d_frames, size_t stride_t, size_t stride_y, int n_frames,
                                  float* d_out, size_t out_stride_t, size_t out_stride_y);
void wass_spatial_filter_destroy(wass_spatial_filter* h);

/* ---- Wavenumber-frequency filter of the gridded cube (beyond the reference; DESIGN.md, "Dispersion filter"):
 * out = real(ifftn(fftn(p) * H)) over the whole nt x ny x nx float32 cube, cell (t, y, x) at cube[t * stride_t + y * stride_y + x]
 * (strides in elements), with the DFT stages of the spectrum on the f32 MFMA and a closing stage that makes the real part only.
 *   prepare  m_c = the fp64 sum of the cell's samples that are not NaN, in frame order, divided by their count (0 for a cell that
 *            is NaN throughout, and for every cell with WASS_KFILTER_NO_CENTRE); p = (float)((double)v - m_c), 0 for a NaN sample
 *   H        real float32 in the un-shifted half layout of np.fft.rfftn, [nt][ny][nx / 2 + 1].  PRECONDITION: H is even,
 *            H[f][ky][kx] == H[-f][-ky][kx] on the columns kx = 0 and, nx even, nx / 2; the other columns stand for their mirror
 *            image as well.  The product is conj(X) * H * w / (nt ny nx) in fp64 with one rounding, w = 2 off those columns.
 *   undo     out = (float)((double)y + m_c) with WASS_KFILTER_RESTORE_MEAN, else y; with WASS_KFILTER_KEEP_NAN a sample that was NaN
 *            is NaN, without it it holds the filtered value; a cell that was NaN throughout is NaN either way
 * An infinite sample is WASS_ERR_INVALID_ARG.  The same input gives the same bits on every run, for host and device memory.
 * create: the handle owns about 3.6 f32 copies of the cube (wass_kfilter_scratch_bytes says how much, without a GPU);
 * WASS_ERR_NO_MEMORY when that is more than 16 GiB or the allocation fails, WASS_ERR_INVALID_ARG for an axis outside 1 .. 8192.
 * set_mask: H from the host.  set_shell: H made on the device from host maps given on the np.fft.fftshift-ed axes: omega[nt],
 * kappa_x[nx], kappa_y[ny], sigma0[ny][nx] doubles and used[ny][nx] bytes.  H = 0 at frequency 0 and at the Nyquist index of every
 * even axis.  A bin of positive frequency (un-shifted 1 <= f <= (nt - 1) / 2) at the shifted indices (p, i, j) is 1 if
 * used[i][j] and f_lo <= omega[p] <= f_hi and |r| <= G, r = (omega[p] - sigma0[i][j]) - (kappa_x[j] * U + kappa_y[i] * V) in that
 * order of operations, else 0; a bin of negative frequency takes the value of its mirror image (-f, -ky, -kx).  complement != 0
 * exchanges 0 and 1 on the bins so decided.  f_lo and f_hi are compared with omega, in its units.  *n_pass (may be NULL) = the bins
 * of the full cube with H = 1.  get_mask: H back to the host.
 * apply: a host cube, returns with out filled; apply_dev: device memory (out may be the cube).  Both wait for the device, since
 * *stats (may be NULL) comes from it: var_in and var_out are the mean squares of p and of the filtered field y over the samples
 * that were not NaN (fp64 sums in a fixed order; NaN without such a sample). */
enum { WASS_KFILTER_RESTORE_MEAN = 1, WASS_KFILTER_KEEP_NAN = 2, WASS_KFILTER_NO_CENTRE = 4 };
typedef struct wass_kfilter_stats {
    double var_in, var_out;
    uint64_t n_nan;             /* NaN samples of the input */
    uint64_t n_empty_cells;     /* cells that are NaN in every frame */
} wass_kfilter_stats;
typedef struct wass_kfilter wass_kfilter;
int wass_kfilter_scratch_bytes(int nt, int ny, int nx, size_t* bytes);
int wass_kfilter_create(wass_ctx* ctx, int nt, int ny, int nx, wass_kfilter** out);
int wass_kfilter_set_mask(wass_kfilter* h, const float* H);
int wass_kfilter_set_shell(wass_kfilter* h, const double* omega, const double* kappa_x, const double* kappa_y, const double* sigma0,
                           const unsigned char* used, double U, double V, double G, double f_lo, double f_hi, int complement,
                           uint64_t* n_pass);
int wass_kfilter_get_mask(wass_kfilter* h, float* H);
int wass_kfilter_apply(wass_kfilter* h, const float* cube, size_t stride_t, size_t stride_y, float* out, size_t out_stride_t,
                       size_t out_stride_y, int flags, wass_kfilter_stats* stats);
int wass_kfilter_apply_dev(wass_kfilter* h, const float* d_cube, size_t stride_t, size_t stride_y, float* d_out, size_t out_stride_t,
                           size_t out_stride_y, int flags, wass_kfilter_stats* stats);
/* Measuring: with set_timing(on != 0) every apply brackets its stages with events, also runs the full closing stage
 * (k_dft_stage<true, true>, the spatial filter's last launch) on the same half spectrum just before k_dft_close, and waits for the
 * device; the result is unchanged.  last_timings: ten floats, milliseconds of the last timed apply: upload + prepare, x, y, t, the
 * product, t, y, the full closing stage, k_dft_close (+ the fold of its sums), the copy to out. */
int wass_kfilter_set_timing(wass_kfilter* h, int on);
int wass_kfilter_last_timings(wass_kfilter* h, float* stage_ms);
void wass_kfilter_destroy(wass_kfilter* h);

/* ---- Visibility map of the gridded cube: wasspost visibilitymap (wasspost.py:495-621, geometry.py:5-100) as an array function.
 * For every frame of a count x H x W float32 cube (cell (t, y, x) at in[t * stride_t + y * stride_y + x], strides in elements) and
 * every cell: zf = in * (float)datascale is the height in metres; the unit ray d from (XX, YY, zf) to the camera `origin` (grid
 * coordinates; XX, YY are H x W doubles with XX[0][1] > XX[0][0] and YY[1][0] > YY[0][0], H, W >= 2); the surface normal from
 * np.gradient(zf, dy, dx) as numpy computes it for a float32 array; angles = (float) degrees(acos(n . d)); mask = 1 where the
 * ray, marched one cell of its dominant axis per step over zf / dx with rounding half to even, meets a cell at least as high
 * as itself before it leaves the grid or rises above the frame's maximum, or where the angle is >= angle_limit (a negative or
 * infinite angle_limit switches that rule off).  The ray, the step and the accumulated position are fp64 in numpy's order of
 * operations: the march is the reference's bit for bit.  NaN cells never occlude, have mask 0 and a NaN angle; a cell exactly
 * under the camera has mask 0 from the march; finite cells at or above the camera keep mask 0 and are counted in *not_upward
 * (the reference asserts there).  mask and angles are count x H x W, tightly packed; occluded[t] = the number of mask cells of
 * frame t (may be NULL, as may not_upward).  Frames are processed `batch` at a time (0: 8), halved until the scratch fits
 * 16 GiB; wass_visibility_scratch_bytes says how much and which batch, without a GPU.  The result does not depend on the batch
 * and is the same bits on every run.  wass_visibility: everything on the host, returns with the outputs filled.
 * wass_visibility_dev: in, XX, YY, mask and angles are device memory (origin, occluded, not_upward stay host memory); the work is
 * enqueued on the context's stream, and the call returns after a synchronisation, when it frees its scratch. */
int wass_visibility_scratch_bytes(int count, int H, int W, int batch, int host, size_t* bytes, int* batch_used);
int wass_visibility(wass_ctx* ctx, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* XX,
                    const double* YY, const double origin[3], double datascale, double angle_limit, int batch, uint8_t* mask,
                    float* angles, uint64_t* occluded, uint64_t* not_upward);
int wass_visibility_dev(wass_ctx* ctx, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* d_XX,
                        const double* d_YY, const double origin[3], double datascale, double angle_limit, int batch, uint8_t* d_mask,
                        float* d_angles, uint64_t* occluded, uint64_t* not_upward);
/* compute_occlusion_mask (geometry.py:21-100) in its general form: one H x W fp64 surface in cell units and an H x W x 3 fp64 ray
 * field; the step of a cell is its ray divided by max(|ray0|, |ray1|), its y component negated if invert_y_axis.  Cells whose
 * ray does not have ray2 > 0 keep mask 0 and are counted in *not_upward.  _dev: ZZ, rays and mask are device memory. */
int wass_occlusion_rays(wass_ctx* ctx, const double* ZZ, const double* rays, int H, int W, int invert_y_axis, uint8_t* mask,
                        uint64_t* not_upward);
int wass_occlusion_rays_dev(wass_ctx* ctx, const double* d_ZZ, const double* d_rays, int H, int W, int invert_y_axis, uint8_t* d_mask,
                            uint64_t* not_upward);

/* ---- Radiance of the gridded cube: wasspost radiance (wasspost.py:813-919), bgimage (:1010-1074) and radiance_threshold
 * (:1079-1145) as array functions.
 *
 * wass_remap_lanczos4: cv::remap(src, dst, map_x, map_y, INTER_LANCZOS4) for CV_8UC1 / CV_32FC1 maps, BORDER_CONSTANT 0:
 * X = cvRound(map_x * 32) (float product, nearest even), the window of 8 x 8 taps starts at (X >> 5) - 3 (saturated to int16
 * first), the 64 int16 weights of phase (Y & 31) * 32 + (X & 31) from OpenCV's fixed-point table (wass_lanczos4_table writes
 * its 1024 x 8 x 8 entries; no GPU needed), int32 sum, (v + 2^14) >> 15 clamped to 0 .. 255; taps outside the picture count 0.
 * A map value that is NaN, infinite or whose product with 32 leaves the int32 range gives 0.  The sides of the picture are
 * below 32767.  Written from knowledge of OpenCV 4.5.5 and not pinned against it.  dst and the maps are dw x dh, tightly packed.
 *
 * wass_radiance: out[t][y][x] = remap(images[t]) / 255 (float32) at mapx = (float)(r_0 / r_2), mapy = (float)(r_1 / r_2) with
 * r_k = ((P[k][0] XX + P[k][1] YY) + P[k][2] zf) + P[k][3] in fp64 and zf = in * (float)datascale in float32; Pcam is the 3 x 4
 * row-major projection into picture pixels.  images: count pictures of Ih x Iw bytes, picture t at images + t * image_stride_t,
 * rows image_stride_y apart; the cube as for wass_visibility; out is count x H x W, tightly packed.  Frames go `batch` at a
 * time (0: 8).  The device form needs no scratch and only enqueues on the context's stream; the host form stages XX, YY and
 * the frames of a batch (wass_radiance_scratch_bytes says how much, without a GPU) and returns with out filled.
 *
 * wass_bgimage: scipy.ndimage.uniform_filter1d(in, size, axis=0, mode='reflect') of the float32 cube, bit for bit as scipy 1.15
 * computes it: the window at t covers t - size / 2 .. t + size - size / 2 - 1, indices reflected half-sample symmetric as often
 * as needed, the sum of the first window in fp64, then sum += in[new] - in[old], out[t] = (float)(sum / size).  A NaN poisons
 * its series from the first window that holds it to the end.  out must not be in.  The host form works in slabs of rows
 * (slab_rows > 0 caps them; the result does not depend on it) under 16 GiB of scratch; the device form needs none.
 *
 * The threshold, per frame and in float32: m = min(Ibg) (NaN if Ibg holds one), Isub = I - (Ibg - m).
 *   wass_radiance_range  bgmin[t] = m, lo[t] / hi[t] = the smallest / largest finite Isub (NaN if there is none),
 *                        nonfinite[t] = the cells of Isub that are NaN or infinite
 *   wass_radiance_hist   counts[t][30] = the histogram of Isub against edges[t][31] as np.histogram counts: the left edge
 *                        inclusive, the last bin closed, the edges themselves deciding; values outside are not counted
 *   wass_radiance_mask   mask[t][y][x] = Isub > thr[t]
 * bgmin, lo, hi, nonfinite, edges, counts and thr are host memory in both forms; I, Ibg (element strides as for the cube) and
 * mask (count x H x W, tightly packed) are host memory or, in the _dev forms, device memory.  Every call returns after a
 * synchronisation.  Integer atomics only: the same input gives the same bits. */
int wass_lanczos4_table(int16_t* out /* 1024 * 64 */);
int wass_remap_lanczos4(wass_ctx* ctx, const uint8_t* src, int sw, int sh, size_t src_stride, const float* map_x, const float* map_y,
                        int dw, int dh, uint8_t* dst);
int wass_remap_lanczos4_dev(wass_ctx* ctx, const uint8_t* d_src, int sw, int sh, size_t src_stride, const float* d_map_x,
                            const float* d_map_y, int dw, int dh, uint8_t* d_dst);
int wass_radiance_scratch_bytes(int count, int H, int W, int Ih, int Iw, int batch, int host, size_t* bytes, int* batch_used);
int wass_radiance(wass_ctx* ctx, const uint8_t* images, size_t image_stride_t, size_t image_stride_y, int Ih, int Iw, const float* in,
                  size_t stride_t, size_t stride_y, int count, int H, int W, const double* XX, const double* YY, const double Pcam[12],
                  double datascale, int batch, float* out);
int wass_radiance_dev(wass_ctx* ctx, const uint8_t* d_images, size_t image_stride_t, size_t image_stride_y, int Ih, int Iw,
                      const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* d_XX,
                      const double* d_YY, const double Pcam[12], double datascale, int batch, float* d_out);
int wass_bgimage_scratch_bytes(int count, int H, int W, int size, int slab_rows, int host, size_t* bytes, int* rows_per_slab);
int wass_bgimage(wass_ctx* ctx, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, int size, int slab_rows,
                 float* out, size_t out_stride_t, size_t out_stride_y);
int wass_bgimage_dev(wass_ctx* ctx, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, int size,
                     int slab_rows, float* d_out, size_t out_stride_t, size_t out_stride_y);
int wass_radiance_threshold_scratch_bytes(int count, int H, int W, int batch, int host, size_t* bytes, int* batch_used);
int wass_radiance_range(wass_ctx* ctx, const float* I, size_t stride_t, size_t stride_y, const float* Ibg, size_t bg_stride_t,
                        size_t bg_stride_y, int count, int H, int W, int batch, float* bgmin, float* lo, float* hi, uint32_t* nonfinite);
int wass_radiance_range_dev(wass_ctx* ctx, const float* d_I, size_t stride_t, size_t stride_y, const float* d_Ibg, size_t bg_stride_t,
                            size_t bg_stride_y, int count, int H, int W, int batch, float* bgmin, float* lo, float* hi,
                            uint32_t* nonfinite);
int wass_radiance_hist(wass_ctx* ctx, const float* I, size_t stride_t, size_t stride_y, const float* Ibg, size_t bg_stride_t,
                       size_t bg_stride_y, int count, int H, int W, int batch, const float* bgmin, const float* edges, uint32_t* counts);
int wass_radiance_hist_dev(wass_ctx* ctx, const float* d_I, size_t stride_t, size_t stride_y, const float* d_Ibg, size_t bg_stride_t,
                           size_t bg_stride_y, int count, int H, int W, int batch, const float* bgmin, const float* edges,
                           uint32_t* counts);
int wass_radiance_mask(wass_ctx* ctx, const float* I, size_t stride_t, size_t stride_y, const float* Ibg, size_t bg_stride_t,
                       size_t bg_stride_y, int count, int H, int W, int batch, const float* bgmin, const float* thr, uint8_t* mask);
int wass_radiance_mask_dev(wass_ctx* ctx, const float* d_I, size_t stride_t, size_t stride_y, const float* d_Ibg, size_t bg_stride_t,
                           size_t bg_stride_y, int count, int H, int W, int batch, const float* bgmin, const float* thr,
                           uint8_t* d_mask);

/* ---- Pyramid upsampling: cv::pyrUp of float32 / float64 pictures, and wasspost radiance --upscalefactor N on it
 * (wasspost.py:840-843, 880-896).
 *
 * wass_pyrup_f32 / _f64: every H x W frame (H, W >= 2) becomes 2^levels H x 2^levels W, levels from 1 to 4, each level OpenCV
 * 4.5.5's scalar pyrUp_ restated from knowledge and not pinned against it: in the element type without contraction, x first (the
 * two ends of a row as OpenCV writes them: r[0] = s[0]*6 + s[1]*2, r[2w-2] = s[w-2] + s[w-1]*7, r[2w-1] = s[w-1]*8; between
 * them r[2j] = (s[j-1] + s[j]*6) + s[j+1] and r[2j+1] = (s[j] + s[j+1])*4), then y in the three-tap form on reflected rows (row
 * -1 is row 1, row H is row H-1), times 1/64.  Strides are in elements, the last axis is contiguous, the frames of out do not
 * overlap; the _dev forms cannot work in place.  Frames go 8 at a time; every level but the last goes through tightly packed
 * scratch, and the host forms stage the input and the result as well (wass_pyrup_scratch_bytes says how much and which batch
 * for elem_size 4 or 8, without a GPU; at most 16 GiB, else the batch is halved).  A side below 2 or levels outside 1 .. 4:
 * WASS_ERR_INVALID_ARG; a side of the result above 65536: WASS_ERR_UNSUPPORTED.  The host forms return with out filled; the
 * _dev forms enqueue on the context's stream and synchronise only when they used scratch (levels > 1).
 *
 * wass_radiance_up: wass_radiance on the grid and the heights upsampled by `levels` levels: zf = in * (float)datascale in
 * float32 first (the rule of wass_radiance), then pyrUp of zf in float32 and of XX, YY in fp64 (once per call), then the
 * projection and the sampler of wass_radiance at every cell of the finer grid.  out is count x 2^levels H x 2^levels W, tightly
 * packed; everything else as for wass_radiance.  Both forms allocate scratch (wass_radiance_up_scratch_bytes) and return after
 * a synchronisation. */
int wass_pyrup_scratch_bytes(int count, int H, int W, int levels, int elem_size, int batch, int host, size_t* bytes, int* batch_used);
int wass_pyrup_f32(wass_ctx* ctx, const float* in, size_t in_stride_t, size_t in_stride_y, int count, int H, int W, int levels, float* out,
                   size_t out_stride_t, size_t out_stride_y);
int wass_pyrup_f32_dev(wass_ctx* ctx, const float* d_in, size_t in_stride_t, size_t in_stride_y, int count, int H, int W, int levels,
                       float* d_out, size_t out_stride_t, size_t out_stride_y);
int wass_pyrup_f64(wass_ctx* ctx, const double* in, size_t in_stride_t, size_t in_stride_y, int count, int H, int W, int levels, double* out,
                   size_t out_stride_t, size_t out_stride_y);
int wass_pyrup_f64_dev(wass_ctx* ctx, const double* d_in, size_t in_stride_t, size_t in_stride_y, int count, int H, int W, int levels,
                       double* d_out, size_t out_stride_t, size_t out_stride_y);
int wass_radiance_up_scratch_bytes(int count, int H, int W, int Ih, int Iw, int levels, int batch, int host, size_t* bytes, int* batch_used);
int wass_radiance_up(wass_ctx* ctx, const uint8_t* images, size_t image_stride_t, size_t image_stride_y, int Ih, int Iw, const float* in,
                     size_t stride_t, size_t stride_y, int count, int H, int W, const double* XX, const double* YY, const double Pcam[12],
                     double datascale, int batch, int levels, float* out);
int wass_radiance_up_dev(wass_ctx* ctx, const uint8_t* d_images, size_t image_stride_t, size_t image_stride_y, int Ih, int Iw,
                         const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* d_XX,
                         const double* d_YY, const double Pcam[12], double datascale, int batch, int levels, float* d_out);

/* ---- Polarimetric set-up of the gridded cube: wasspost polarimetric_setup (wasspost.py:627-805), clip and zeromean as array
 * functions.
 *
 * wass_remap_linear_f32: cv::remap(src, dst, map_x, map_y, INTER_LINEAR) for CV_32FC1 / CV_32FC1 maps, BORDER_CONSTANT 0:
 * X = cvRound(map_x * 32) (float product, nearest even), the window of 2 x 2 taps at (X >> 5, Y >> 5) (saturated to int16), the
 * four float32 weights of phase (Y & 31) * 32 + (X & 31) (wass_bilinear_table_f32 writes the 1024 x 2 x 2 table, w[ky][kx] =
 * ty[ky] * tx[kx] with t = (1 - f / 32, f / 32); no GPU needed), ((v00 w00 + v01 w01) + v10 w10) + v11 w11 in float32 without
 * contraction; each tap outside the picture counts 0, NaN and infinite samples propagate.  A map value that is NaN, infinite
 * or whose product with 32 leaves the int32 range gives 0.  The sides of the picture are below 32767; src_stride is in
 * elements.  Written from knowledge of OpenCV 4.5.5 and not pinned against it.  dst and the maps are dw x dh, tightly packed.
 *
 * wass_polarimetric: per frame t and cell, zf = in * (float)datascale, (u, v) = the projection of wass_radiance in fp64, the
 * camera-frame ray q / |q| with q = ((Kinv[r][0] u + Kinv[r][1] v) + Kinv[r][2]), the mask and the incident angle of
 * wass_visibility (origin, angle_limit: negative or infinite = no angle rule), the three pictures of stokes sampled with
 * wass_remap_linear_f32 at ((float)u, (float)v) and set to NaN where the mask is 1, DOLP = sqrt(S1^2 + S2^2) / S0 in float32,
 * the unit normal (-sx, -sy, 1) / |.| from the float32 slopes of np.gradient.  stokes: picture k of frame t at
 * stokes + t * stokes_stride_t + k * stokes_stride_c, rows stokes_stride_y apart (elements); the cube as for wass_visibility.
 * acc holds 8 * H * W doubles, [Savg H x W x 3 | Navg H x W x 3 | Zavg H x W | valid H x W]: the frames are ADDED to it in order,
 * one fp64 addition per frame and value (nan_to_num(S), the normal, zf, 1 - mask), so the caller zeroes it before the first
 * call and may split a sequence over calls.  With total_frames > 0 the call ends the sequence: Savg / valid, Navg / |Navg|,
 * Zavg / total_frames, in place.  out (may be NULL) names the per-frame results wanted, each count frames, tightly packed; NULL
 * members are not produced.  occluded[count] (may be NULL) and *not_upward as for wass_visibility; if *not_upward is not 0 the
 * sequence is not ended.  Frames go `batch` at a time (0: 8).  The host form stages a batch (wass_polarimetric_scratch_bytes says
 * how much, without a GPU; outputs = the WASS_POL_* bits of the results wanted); the device form needs scratch only for what
 * the visibility map needs and for S, the mask and the angles where they are not wanted.  Both return after a synchronisation.
 *
 * wass_clip_cube: out = min(max(in, lo), hi) in float32, NaN kept; *vmin, *vmax = the range of the values of out that are not
 * NaN (NaN if there are none).  wass_zeromean: per cell the fp64 sum of the frames in order, divided by count; out =
 * (float)((double)in - mean).  out may be in.  Strides in elements; _dev: in and out are device memory. */
#define WASS_POL_S 1
#define WASS_POL_OCCLUSION 2
#define WASS_POL_ANGLES 4
#define WASS_POL_DOLP 8
#define WASS_POL_NORMALS 16
#define WASS_POL_RAYS_CAM 32
typedef struct wass_pol_params {
    double Pcam[12];        /* projection into picture pixels, row-major 3 x 4 */
    double Kinv[9];         /* inverse of the camera's intrinsic matrix, row-major */
    double origin[3];       /* the camera in grid coordinates */
    double datascale;
    double angle_limit;     /* degrees */
    int batch;
    int total_frames;       /* 0: the sequence goes on */
} wass_pol_params;
typedef struct wass_pol_out {
    float* S;               /* [count][H][W][3] */
    uint8_t* occlusion;     /* [count][H][W] */
    float* angles;          /* [count][H][W] */
    float* dolp;            /* [count][H][W] */
    double* normals;        /* [count][H][W][3] */
    double* rays_cam;       /* [count][3][H * W] */
} wass_pol_out;
int wass_bilinear_table_f32(float* out /* 1024 * 4 */);
int wass_remap_linear_f32(wass_ctx* ctx, const float* src, int sw, int sh, size_t src_stride, const float* map_x, const float* map_y,
                          int dw, int dh, float* dst);
int wass_remap_linear_f32_dev(wass_ctx* ctx, const float* d_src, int sw, int sh, size_t src_stride, const float* d_map_x,
                              const float* d_map_y, int dw, int dh, float* d_dst);
int wass_polarimetric_scratch_bytes(int count, int H, int W, int Ih, int Iw, int batch, int host, int outputs, size_t* bytes,
                                    int* batch_used);
int wass_polarimetric(wass_ctx* ctx, const float* stokes, size_t stokes_stride_t, size_t stokes_stride_c, size_t stokes_stride_y, int Ih,
                      int Iw, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, const double* XX,
                      const double* YY, const wass_pol_params* params, double* acc, const wass_pol_out* out, uint64_t* occluded,
                      uint64_t* not_upward);
int wass_polarimetric_dev(wass_ctx* ctx, const float* d_stokes, size_t stokes_stride_t, size_t stokes_stride_c, size_t stokes_stride_y,
                          int Ih, int Iw, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W,
                          const double* d_XX, const double* d_YY, const wass_pol_params* params, double* d_acc,
                          const wass_pol_out* out, uint64_t* occluded, uint64_t* not_upward);
int wass_clip_cube(wass_ctx* ctx, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, float lo, float hi,
                   float* out, size_t out_stride_t, size_t out_stride_y, float* vmin, float* vmax);
int wass_clip_cube_dev(wass_ctx* ctx, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, float lo, float hi,
                       float* d_out, size_t out_stride_t, size_t out_stride_y, float* vmin, float* vmax);
int wass_zeromean(wass_ctx* ctx, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, float* out,
                  size_t out_stride_t, size_t out_stride_y);
int wass_zeromean_dev(wass_ctx* ctx, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, float* d_out,
                      size_t out_stride_t, size_t out_stride_y);

/* ---- Wave-by-wave statistics of the gridded cube (beyond the reference: DESIGN.md "Wave-by-wave statistics" is the
 * specification).  For the series z[0 .. count - 1] of every cell of a count x H x W float32 cube (strides in elements, as for
 * wass_sosfiltfilt), in fp64, every product, quotient and sum rounded on its own, sums first frame to last:
 *   mean = sum(z) / count; eta = (z - mean) * datascale, or z * datascale with demean == 0; the moments sum(eta^2) / count,
 *   sum(eta^2 * eta) / count, sum(eta^2 * eta^2) / count; the largest and the smallest eta;
 *   an up-crossing at i where eta[i] < 0 <= eta[i + 1], at tau = i + eta[i] / (eta[i] - eta[i + 1]) samples; crossing ==
 *   WASS_WS_DOWN looks for the up-crossings of -eta.  Wave k spans the samples after crossing k up to crossing k + 1: H_k = its
 *   largest minus its smallest eta, T_k = (tau[k + 1] - tau[k]) * dt.  With C crossings there are Nw = max(C - 1, 0) waves.
 *   Over the waves in time order: the means of H_k and of H_k^2, the largest H_k and the T_k of the first wave that has it,
 *   Tz = ((tau[C - 1] - tau[0]) * dt) / Nw, and the means of H_k and T_k over the n13 = (Nw + 2) / 3 waves with the largest
 *   H_k (of equal heights at the cut the earlier wave is taken; the sums run in time order over the waves taken).
 * fields holds WASS_WS_NFIELDS maps of H x W doubles in the order of the enum; n_cross H x W int32 = C.  A series with a sample
 * that is not finite gives NaN in every field and -1 in n_cross, and touches no other cell; the wave fields are NaN where
 * Nw == 0.  With hist_bins > 0 every wave of every such series is counted in hist[min((int)floor(H_k / hist_width),
 * hist_bins - 1)]; hist is zeroed first.  WASS_ERR_INVALID_ARG: count < 1, dt not positive or not finite, datascale not
 * finite, another crossing, hist_bins < 0, hist_bins > 0 with hist_width <= 0.
 * Rows go in slabs of at most slab_rows (0: as many as fit 16 GiB of scratch): 2 * (count / 2) * rows * W * 8 bytes for the
 * waves, and for the host form count * rows * W * 4 for the cube, (WASS_WS_NFIELDS * 8 + 4) * rows * W for the results and
 * hist_bins * 8, each part rounded up to 256 bytes; wass_wavestats_scratch_bytes says how much and how many rows, without a
 * GPU, and checks the same arguments.  The result does not depend on the slab height and is the same bits on every run.
 * _dev: in, fields, n_cross and hist are device memory.  Both forms return after a synchronisation. */
enum {
    WASS_WS_MEAN = 0,      /* mean * datascale */
    WASS_WS_M2,
    WASS_WS_M3,
    WASS_WS_M4,
    WASS_WS_ETA_MAX,
    WASS_WS_ETA_MIN,
    WASS_WS_H_MEAN,
    WASS_WS_H_SQMEAN,
    WASS_WS_H_MAX,
    WASS_WS_T_HMAX,
    WASS_WS_T_Z,
    WASS_WS_H_13,
    WASS_WS_T_13,
    WASS_WS_NFIELDS
};
#define WASS_WS_UP 0
#define WASS_WS_DOWN 1
int wass_wavestats_scratch_bytes(int count, int H, int W, double dt, double datascale, int crossing, int hist_bins, double hist_width,
                                 int slab_rows, int host, size_t* bytes, int* rows_per_slab);
int wass_wavestats(wass_ctx* ctx, const float* in, size_t stride_t, size_t stride_y, int count, int H, int W, double dt, double datascale,
                   int crossing, int demean, int hist_bins, double hist_width, int slab_rows, double* fields, int32_t* n_cross,
                   uint64_t* hist);
int wass_wavestats_dev(wass_ctx* ctx, const float* d_in, size_t stride_t, size_t stride_y, int count, int H, int W, double dt,
                       double datascale, int crossing, int demean, int hist_bins, double hist_width, int slab_rows, double* d_fields,
                       int32_t* d_n_cross, uint64_t* d_hist);

/* ---- Spectral products of the 3-D spectrum (beyond the reference: DESIGN.md "Spectral products" is the specification).
 * S is an nt x ny x nx fp64 cube, dense, as wass_spec3d_finish[_dev] leaves it (fftshifted); p0 is its first frequency above
 * zero, and frequencies p0 .. nt - 1 are the positive half.  v = S * scale (scale > 0) is one rounding; every sum below is fp64,
 * every product and sum rounded on its own, in ONE order that depends on nt, ny, nx, p0 and the labels alone.  A label map is
 * ny x nx int32 in host memory, -1 = unused, else 0 .. n - 1; the host computes it (no atan2, sqrt or tanh runs on the device).
 * block_sum(x[0 .. 255]) below is the tree for o = 128, 64, .. 1: x[t] += x[t + o] for t < o.
 *   T[p - p0][b] = block_sum over t of (the cells c_t, c_(t + 256), .. of label b's cells c_0 < c_1 < .. in raster order, added in
 *                  that order from 0.0): T_dir with lab_dir (nf x n_dir, nf = nt - p0), T_k with lab_k (nf x n_k); 0 for an empty label
 *   E2[i][j]     = v summed over p = p0 .. nt - 1 in that order from 0.0, for every cell, used or not
 *   peak         = the largest v over p >= p0 (wass_specprod_peak_dev: pa <= p < pb) and the cells with lab_dir (labels) >= 0;
 *                  *peak_index = (p ny + i) nx + j of the lowest such index among equal values; NaN and -1 if no cell is used
 * A v of the positive half that is negative or not finite: WASS_ERR_INVALID_ARG (the kernels set a flag; the outputs are then
 * not defined); the other half is never read.  A label outside -1 .. n - 1: WASS_ERR_INVALID_ARG.
 * wass_specprod_tables takes S in host memory and stages it in slabs of at most `slab` frequencies (0: as many as fit 16 GiB of
 * scratch together with the tables); the result does not depend on the slab.  _dev reads S in place.  All outputs are host
 * memory.  wass_specprod_scratch_bytes says how much device memory a call takes and how many frequencies go per slab, without a
 * GPU, and checks the same arguments.
 *
 * wass_specprod_current_sums_dev: the weighted normal equations of the current fit.  omega[nt], kappa_x[nx], kappa_y[ny],
 * sigma0[ny][nx] and labels are host memory.  A bin (p, i, j) is taken when labels[i][j] >= 0, pa <= p < pb, w >= threshold_value
 * and |r| <= gate_value (pass infinity for no gate), with w = v, kx = kappa_x[j], ky = kappa_y[i], d = omega[p] - sigma0[i][j],
 * r = d - (kx * U + ky * V).  sums[WASS_SPECPROD_*]: AXX = sum (w kx) kx, AXY = sum (w kx) ky, AYY = sum (w ky) ky,
 * BX = sum (w kx) d, BY = sum (w ky) d, SW = sum w, SR2 = sum (w r) r; *n_bins the bins taken (exact).  Order: per cell over
 * p ascending from 0.0; block_sum over the 256 cells c = 256 g + t of group g (raster order, an unused cell or one past the map
 * adds 0.0); then block_sum over t of (groups t, t + 256, .. added in that order from 0.0).  A bin of a used cell in pa .. pb - 1
 * that is negative or not finite: WASS_ERR_INVALID_ARG.
 * Every call returns after a synchronisation and gives the same bits on every run. */
enum {
    WASS_SPECPROD_AXX = 0,
    WASS_SPECPROD_AXY,
    WASS_SPECPROD_AYY,
    WASS_SPECPROD_BX,
    WASS_SPECPROD_BY,
    WASS_SPECPROD_SW,
    WASS_SPECPROD_SR2,
    WASS_SPECPROD_NSUMS
};
int wass_specprod_scratch_bytes(int nt, int ny, int nx, int p0, int n_dir, int n_k, int slab, int host, size_t* bytes, int* freqs_per_slab);
int wass_specprod_tables(wass_ctx* ctx, const double* S, int nt, int ny, int nx, int p0, double scale, const int32_t* lab_dir, int n_dir,
                         const int32_t* lab_k, int n_k, int slab, double* T_dir, double* T_k, double* E2, double* peak_value,
                         int64_t* peak_index);
int wass_specprod_tables_dev(wass_ctx* ctx, const double* d_S, int nt, int ny, int nx, int p0, double scale, const int32_t* lab_dir, int n_dir,
                             const int32_t* lab_k, int n_k, double* T_dir, double* T_k, double* E2, double* peak_value, int64_t* peak_index);
int wass_specprod_peak_dev(wass_ctx* ctx, const double* d_S, int nt, int ny, int nx, int p0, int pa, int pb, double scale,
                           const int32_t* labels, double* peak_value, int64_t* peak_index);
int wass_specprod_current_sums_dev(wass_ctx* ctx, const double* d_S, int nt, int ny, int nx, int pa, int pb, double scale,
                                   const int32_t* labels, const double* omega, const double* kappa_x, const double* kappa_y,
                                   const double* sigma0, double U, double V, double threshold_value, double gate_value, double* sums,
                                   int64_t* n_bins);

/* ---- Feature matcher: the game-theoretic inlier selection of wass_match (src/wass_match/GTMatcher.cpp, iidyn.cpp) as array
 * functions.  A feature is four float32, x y scale angle (the head of a record of FeatureSet::save); a candidate is a pair of
 * int32, (feature of A, feature of B).
 *
 * wass_match_knn: for every descriptor of A (na x d float32) the kk = min(k, nb) descriptors of B (nb x d) at the smallest squared
 * L2 distance, the float32 differences squared and summed in index order without contraction; by increasing distance, equal
 * distances by increasing index.  idx and dist are na x kk.  An exact search: the reference asks a randomised kd-forest
 * (FeatureSet.cpp:452-468), whose limit this is.  1 <= k <= WASS_MATCH_MAX_K, 1 <= d <= WASS_MATCH_MAX_DESC.  A distance that is NaN
 * is never a neighbour; a feature with fewer than kk neighbours left gets idx -1 and an infinite distance for the rest.
 *
 * wass_match_payoff: the n x n fp64 matrix of compute_payoff_matrix (:219-250).  Per candidate compute_affine (:69-97) in fp64 with
 * the float32 positions, scales and angles widened where the reference widens them (ang_diff's two loops included); entry (i, j) =
 * exp(-lambda * max(e_ij, e_ji)), e_ij the squared distance from candidate j's target to candidate i's transform of candidate j's
 * source; 0 where the two share a source or a target, the diagonal included.  The matrix is symmetric bit for bit.  A candidate
 * outside its feature set, or two angles more than 1e4 apart (the reference's loops would not end) or not numbers:
 * WASS_ERR_INVALID_ARG after the launch, which reads nothing out of bounds.
 *
 * wass_match_iidyn: gt_iidyn (iidyn.cpp:520-596) from the start x (or, with uniform_start, from gt_create_population's, which is
 * uniform: its rand() / RAND_MAX is an integer division), one workgroup of 1024 threads per problem with x and Ax in registers.
 * A step keeps the reference's order: selectStrategy (the first largest Ax; the first smallest Ax among x > 0), the Nash error, the
 * mu / do_remove cases, scale, x[idx], simplexify, linear_comb as alfa * (x - y) + y.  Sums and extrema are reduced in one fixed
 * tree that depends on n alone (a thread's elements in index order, a butterfly over the wave, the waves in order), so a problem
 * gives the same bits alone and in any batch; the reference sums sequentially, which moves the population by rounding only.
 * toll is squared as the reference squares it.  *steps = the steps taken, *err = the last Nash error (DBL_MAX when max_iters is
 * 0).  Where the reference would read A[-size - 1] (no strategy qualifies: a population that is all zero or NaN) the loop ends.
 * group[i] = x[i] > max(x) * pop_threshold (match_group :273-293), *group_size their number.  n <= WASS_MATCH_MAX_N.
 *
 * The _dev forms take `batch` problems in device memory: problem p has n[p] candidates (n, na, nb: host arrays) and lives at
 * base + p * stride, strides in elements (float32 for features, int32 for candidates, fp64 for A and x, bytes for group); its
 * matrix is n[p] x n[p], tightly packed.  With batch == 1 the strides are not read.  wass_match_round_dev is one round of the
 * matcher for the batch: payoff, uniform start, dynamics, group.  wass_match_scratch_bytes: the device memory such a round takes
 * for `batch` problems of at most n_max candidates, the caller's arrays (A, x, group, candidates) and the context's own together;
 * no GPU needed.  Every call returns after a synchronisation. */
#define WASS_MATCH_MAX_N 8192
#define WASS_MATCH_MAX_K 8
#define WASS_MATCH_MAX_DESC 256
int wass_match_scratch_bytes(int batch, int n_max, size_t* bytes);
int wass_match_knn(wass_ctx* ctx, const float* desc_a, int na, const float* desc_b, int nb, int d, int k, int32_t* idx, float* dist);
int wass_match_knn_dev(wass_ctx* ctx, const float* d_desc_a, int na, const float* d_desc_b, int nb, int d, int k, int32_t* d_idx,
                       float* d_dist);
int wass_match_payoff(wass_ctx* ctx, const float* fa, int na, const float* fb, int nb, const int32_t* cand, int n, double lambda,
                      double* A);
int wass_match_payoff_dev(wass_ctx* ctx, const float* d_fa, size_t fa_stride, const float* d_fb, size_t fb_stride, const int32_t* d_cand,
                          size_t cand_stride, const int* n, const int* na, const int* nb, int batch, double lambda, double* d_A,
                          size_t A_stride);
int wass_match_iidyn(wass_ctx* ctx, const double* A, int n, double* x, int uniform_start, double toll, int max_iters,
                     double pop_threshold, int* steps, double* err, uint8_t* group, int* group_size);
int wass_match_iidyn_dev(wass_ctx* ctx, const double* d_A, size_t A_stride, double* d_x, size_t x_stride, int uniform_start, const int* n,
                         int batch, double toll, int max_iters, double pop_threshold, int* steps, double* err, uint8_t* d_group,
                         size_t group_stride, int* group_size);
int wass_match_round_dev(wass_ctx* ctx, const float* d_fa, size_t fa_stride, const float* d_fb, size_t fb_stride, const int32_t* d_cand,
                         size_t cand_stride, const int* n, const int* na, const int* nb, int batch, double lambda, double toll,
                         int max_iters, double pop_threshold, double* d_A, size_t A_stride, double* d_x, size_t x_stride, int* steps,
                         double* err, uint8_t* d_group, size_t group_stride, int* group_size);

/* ---- Essential-matrix filter: what wass_match does after matches_unfiltered.txt (wass_match.cpp:250-358), cv::findEssentialMat's
 * RANSAC as array functions.  A match is two points in normalised coordinates, x0 = K0^-1 (u0, v0, 1) and x1 = K1^-1 (u1, v1, 1),
 * two fp64 each; E (row-major 3 x 3 fp64) satisfies x1' E x0 = 0.  Everything is fp64 without contraction.
 *
 * wass_epi_solve5: a sample is five int32 indices into a pair's matches; it gives up to WASS_EPI_MAX_SOL essential matrices (the
 * five-point problem, Nister 2004): the null space of the 5 x 9 constraint matrix (Gauss-Jordan with complete pivoting, then
 * Gram-Schmidt), the ten cubic constraints det E = 0 and 2 E E' E - tr(E E') E = 0 on E = x X + y Y + z Z + W, Gauss-Jordan with
 * partial pivoting, the degree-10 polynomial in z, its real roots (those in [-1, 1], and 1 / z in [-1, 1] from the reversed
 * polynomial; each isolated between the roots of the derivative before it and bisected), x and y from the null vector of the 3 x 3
 * polynomial matrix at the root, three Gauss-Newton steps on the ten constraints.  Per sample: nsol, and ten slots of which the
 * first nsol hold the solutions scaled to Frobenius norm 1, by ascending z, the others zero.  A solution with an entry that is not
 * finite is dropped; a rank-deficient sample gives the finite solutions it has, possibly none, never a NaN.  The output depends on
 * the sample alone: not on the launch, the batch or the other samples.  One hypothesis per thread, workgroups of 64.
 *
 * wass_epi_score: the inlier count of every model over every match of its pair.  With a = x0, b = x1 and E row-major:
 *     l0 = (E0 ax + E1 ay) + E2    l1 = (E3 ax + E4 ay) + E5    l2 = (E6 ax + E7 ay) + E8            (E x0)
 *     r0 = (E0 bx + E3 by) + E6    r1 = (E1 bx + E4 by) + E7                                         (E' x1)
 *     num = (bx l0 + by l1) + l2   den = ((l0 l0 + l1 l1) + r0 r0) + r1 r1
 *     err = (float)((num num) / den)                                            the squared Sampson distance
 * every product and sum rounded on its own in fp64; a match is an inlier when err <= (float)(t * t).  A comparison with NaN is
 * false: a NaN match, and every match of a model of zeros, is no inlier.  counts are int32 and exact.  d_nsol (may be null): the
 * models are rounds x 10 slots of wass_epi_solve5 and a slot at or above its sample's nsol gets the count -1.
 *
 * wass_epi_mask: mask (uint8) and err (float32) of one model per pair, the same arithmetic.
 *
 * wass_epi_find: the chain solve5 -> score -> best -> mask with no host synchronisation in between.  The best model has the
 * largest count; of equal counts the lowest model index sample * 10 + solution wins (the reference's strict >).  E (host, 9 per
 * pair), best_index and best_count (host, one per pair; index -1 and a zero E when no sample gave a solution), and the best
 * model's mask and err in device memory.
 *
 * All forms take `batch` pairs in device memory: pair p has m[p] matches and the threshold t[p] (m, t: host arrays) and lives at base + p * stride; strides
 * in elements (fp64 for points, int32 for samples, bytes / float32 for mask / err); every pair has `rounds` samples or `nmodels`
 * models, tightly packed.  With batch == 1 the strides are not read.  A pair of a batch gives bit for bit what it gives alone.  A
 * sample index outside [0, m[p]) is WASS_ERR_INVALID_ARG after the launch, which reads nothing out of bounds.
 * 5 <= m[p] <= WASS_EPI_MAX_M, 1 <= rounds <= WASS_EPI_MAX_ROUNDS.  wass_epi_scratch_bytes: the context's own device memory for
 * wass_epi_find; no GPU needed.  Every call returns after a synchronisation. */
#define WASS_EPI_MAX_SOL 10
#define WASS_EPI_MAX_ROUNDS 65536
#define WASS_EPI_MAX_M (1 << 22)
int wass_epi_scratch_bytes(int batch, int rounds, size_t* bytes);
int wass_epi_solve5_dev(wass_ctx* ctx, const double* d_x0, const double* d_x1, size_t pt_stride, const int32_t* d_samples,
                        size_t sample_stride, const int* m, int rounds, int batch, double* d_E, int32_t* d_nsol);
int wass_epi_score_dev(wass_ctx* ctx, const double* d_E, int nmodels, const int32_t* d_nsol, const double* d_x0, const double* d_x1,
                       size_t pt_stride, const int* m, const double* t, int batch, int32_t* d_counts);
int wass_epi_mask_dev(wass_ctx* ctx, const double* d_E, const double* d_x0, const double* d_x1, size_t pt_stride, const int* m, const double* t,
                      int batch, uint8_t* d_mask, float* d_err, size_t out_stride);
int wass_epi_find_dev(wass_ctx* ctx, const double* d_x0, const double* d_x1, size_t pt_stride, const int32_t* d_samples,
                      size_t sample_stride, const int* m, const double* t, int rounds, int batch, double* E, int* best_index, int* best_count,
                      uint8_t* d_mask, float* d_err, size_t out_stride);

/* ---- Autocalibration: what wass_autocalibrate does between the matcher and the stereo stage (src/wass_autocalibrate/): the choice
 * among the four poses of an essential matrix and the bundle adjustment of two cameras over N points seen by both (sba's
 * sba_motstr_levmar_x with no constant frame).  Everything is fp64 without contraction; every product, sum, quotient and square
 * root below is rounded on its own, in the order the parentheses give.
 *
 * wass_ac_triangulate: R4 (host, 4 x 9 row-major) and T4 (host, 4 x 3) are the candidates; one thread per (candidate, match).  With
 * p = x0, q = x1 of the match, the 4 x 3 system has the rows (-1, 0, p0), (0, -1, p1), r2 and r3 and the right side (0, 0, b2, b3):
 *     r2k = q0 R[2][k] - R[0][k]     r3k = q1 R[2][k] - R[1][k]     b2 = T0 - T2 q0     b3 = T1 - T2 q1
 *     a = (1 + r20 r20) + r30 r30    b = r20 r21 + r30 r31          c = (r20 r22 - p0) + r30 r32
 *     d = (1 + r21 r21) + r31 r31    e = (r21 r22 - p1) + r31 r32   f = ((p0 p0 + p1 p1) + r22 r22) + r32 r32
 *     yk = r2k b2 + r3k b3
 *     C00 = d f - e e   C01 = c e - b f   C02 = b e - c d   C11 = a f - c c   C12 = b c - a e   C22 = a d - b b
 *     det = (a C00 + b C01) + c C02
 *     X = ((C00 y0 + C01 y1) + C02 y2) / det   Y = ((C01 y0 + C11 y1) + C12 y2) / det   Z = ((C02 y0 + C12 y1) + C22 y2) / det
 * det zero or not finite: the point is NaN.  d_pts: 4 x m x 3; counts (host, 4): per candidate the matches with mask != 0 and
 * Z > 1 (a NaN counts nowhere), exact.
 *
 * A camera is 15 doubles: R0 (9, row-major, fixed), v (3) and t (3).  With s = (v0 v0 + v1 v1) + v2 v2, w = sqrt(1 - s) (NaN for
 * |v| > 1), Rl[r][k] = I[r][k] + 2 (w [v]x[r][k] + (v_r v_k - s I[r][k])) and Rj[r][k] = (Rl[r][0] R0[0][k] + Rl[r][1] R0[1][k]) +
 * Rl[r][2] R0[2][k] (host arithmetic), a point M projects to
 *     X_r = ((Rj[r][0] M0 + Rj[r][1] M1) + Rj[r][2] M2) + t_r      iz = 1 / X2      px = X0 iz      py = X1 iz
 * and the residual is (ex, ey) = (u - px, v - py) of the measured (u, v): obs holds (u0, v0, u1, v1) per point, pts (X, Y, Z).
 * The Jacobian rows, with Y_r = (R0[r][0] M0 + R0[r][1] M1) + R0[r][2] M2, c = v x Y (c0 = v1 Y2 - v2 Y1, ...),
 * h = (v0 Y0 + v1 Y1) + v2 Y2, g_r = w Y_r + c_r, G_r = (1 / w) c_r + Y_r:
 *     D[r][k] = 2 ((h I[r][k] - G_r v_k) - [g]x[r][k])                                   dX / dv; off the diagonal 0 - G_r v_k
 *     ax_k = iz (D[0][k] - px D[2][k])   ay_k = iz (D[1][k] - py D[2][k])                k = 0 .. 2
 *     ax_3..5 = iz, 0, -(px iz)          ay_3..5 = 0, iz, -(py iz)
 *     bx_k = iz (Rj[0][k] - px Rj[2][k]) by_k = iz (Rj[1][k] - py Rj[2][k])
 * and per point, camera 0 first: V_kl = (bx_k bx_l + by_k by_l)_0 + (...)_1, eb_k = (bx_k ex + by_k ey)_0 + (...)_1,
 * W_j[a][k] = ax_a bx_k + ay_a by_k, |e_i|^2 = (ex ex + ey ey)_0 + (...)_1; per camera U_j[a][b] = sum_i ax_a ax_b + ay_a ay_b and
 * ea_j[a] = sum_i ax_a ex + ay_a ey.
 *
 * wass_ac_linearize: d_lin (may be null) gets WASS_AC_LIN_ROWS rows of n: ex0 ey0 ex1 ey1, V (00 01 02 11 12 22), eb (3),
 * W_0 (18, a-major), W_1 (18).  sums (host, WASS_AC_LIN_SUMS): the lower triangles of U_0 and U_1 by rows (21 each), ea (12),
 * |e|^2, max_i,k |eb_i,k| and max_i,k V_i,kk.
 *
 * wass_ac_step: one Schur step at mu from the linearisation at (cams, pts).  Per point Vi = (V_i + mu I)^-1 by the cofactor
 * rule (as C00 .. det above with a, d, f the damped diagonal; Vi = C (1 / det)), Y_p = (W_p0 Vi_0k + W_p1 Vi_1k) + W_p2 Vi_2k
 * for the 12 stacked rows of W_0, W_1, the sums T_pq = sum_i (Y_p0 W_q0 + Y_p1 W_q1) + Y_p2 W_q2 and r_p = sum_i (Y_p0 eb0 +
 * Y_p1 eb1) + Y_p2 eb2; S = diag(U_0 + mu I, U_1 + mu I) - T and rhs = ea - r on the host (S: 144, rhs: 12), a Cholesky
 * factorisation by rows and two triangular solves give da (12: v and t of camera 0, then of camera 1).  *ok = 0 when a pivot or
 * an entry of da is not positive or not finite: a rejected step, with da and scal zero.  Otherwise per point
 *     g_k = eb_k - (((W[0][k] da_0 + W[1][k] da_1) + ...) + W[11][k] da_11)     db_r = (Vi_r0 g0 + Vi_r1 g1) + Vi_r2 g2
 * d_db and d_pts_new = pts + db (n x 3 each, may be null), cams_new = cams with da added to v and t (host, 30), and scal (host,
 * 4): |e_new|^2 at the candidate, |dp|^2, |p|^2 and dL = dp' (mu dp + J'e), each the points' sum and then the cameras' terms.
 *
 * wass_ac_error: |e|^2 at (cams, pts); d_res (may be null) 4 rows of n.
 *
 * wass_ac_bundle: the Levenberg-Marquardt loop of sba on the host, restated from knowledge: mu = 1e-3 max diag(J'J),
 * additive damping, Nielsen's update, thresholds 1e-12.  cams (host, 30) and d_pts are updated in place to the last accepted
 * step.  info (host, 8): initial and final |e|^2, iterations, stop reason (1 gradient, 2 step, 3 iterations, 4 step too large, 5
 * damping overflow, 6 error, 7 not finite), mu, the gradient's infinity norm, |dp|^2 of the last solve, solves.
 *
 * Reductions: a workgroup is one wave of 64 and sums with the tree l += l + 32, 16, 8, 4, 2, 1 (a lane past n adds 0.0); the
 * workgroups are then added in ascending order.  The per-point results do not depend on n.  1 <= n, m <= WASS_AC_MAX_N.
 * wass_ac_scratch_bytes: the context's device memory for n points; no GPU needed.  Every call returns after a synchronisation. */
#define WASS_AC_LIN_ROWS 49
#define WASS_AC_LIN_SUMS 57
#define WASS_AC_MAX_N (1 << 22)
int wass_ac_scratch_bytes(int n, size_t* bytes);
int wass_ac_triangulate_dev(wass_ctx* ctx, const double* d_x0, const double* d_x1, const uint8_t* d_mask, int m, const double* R4, const double* T4,
                            double* d_pts, int32_t* counts);
int wass_ac_linearize_dev(wass_ctx* ctx, const double* cams, const double* d_pts, const double* d_obs, int n, double* d_lin, double* sums);
int wass_ac_step_dev(wass_ctx* ctx, const double* cams, const double* d_pts, const double* d_obs, int n, double mu, double* S, double* rhs,
                     double* da, double* d_db, double* d_pts_new, double* cams_new, double* scal, int* ok);
int wass_ac_error_dev(wass_ctx* ctx, const double* cams, const double* d_pts, const double* d_obs, int n, double* d_res, double* err);
int wass_ac_bundle_dev(wass_ctx* ctx, double* cams, double* d_pts, const double* d_obs, int n, int max_iters, double* info);

/* Coll-1: NaN-aware mean of per-frame planes (np.nanmean of planes.txt,
 * gridding/wassgridsurface/wassgridsurface.py:672-678).  Reduces
 * [sum a, sum b, sum c, sum d, n_valid] into acc5 (caller all-reduces acc5
 * over ranks with RCCL/torch.distributed, then calls wass_planes_mean_finish). */
void wass_planes_mean_accumulate(const double* planes, int n, double acc5[5]);
void wass_planes_mean_finish(const double acc5[5], double mean_out[4], int* n_valid);

/* Coll-1 as a collective: one rank per GPU (one process per GPU, one context per process).  Rank 0 draws an id
 * (ncclGetUniqueId, 128 bytes) and hands it to the other ranks by whatever means the launcher has (pipe, file, env);
 * every rank then calls wass_coll_init and, once per sequence, wass_coll_allreduce_sum_f64 on the acc5 of
 * wass_planes_mean_accumulate -- an RCCL all-reduce (ncclSum, fp64) over xGMI on the context's stream, in place on
 * host values, followed by wass_planes_mean_finish.  librccl is loaded on first use; WASS_ERR_DEVICE if it is
 * missing.  Replaces: the shared output/planes.txt of cli/wasscli/wasscli.py:320,341-343 as the means of agreeing
 * on the sequence's mean plane.  The communicator is destroyed with the context. */
int wass_coll_unique_id(unsigned char id_out[128]);
int wass_coll_init(wass_ctx* ctx, int rank, int world, const unsigned char id[128]);
int wass_coll_allreduce_sum_f64(wass_ctx* ctx, double* values, int count /* <= 64 */);

/* ---- rectification: rectify() of wass_stereo.cpp:447-613 ------------------------
 * Rig-constant host math (no GPU work, usable without a context): */

/* cv::stereoRectify(K_left, 0, K_right, 0, size, R, T, R1, R2, P1, P2, Q, flags=0, alpha, size, &roi1, &roi2)
 * as called at wass_stereo.cpp:541 (Bouguet's algorithm, zero distortion).  3x3 / 3x4 row-major doubles,
 * roi = {x, y, width, height}.  Returns WASS_ERR_INVALID_ARG for a zero baseline. */
int wass_stereo_rectify(const double K_left[9], const double K_right[9], int width, int height, const double R[9],
                        const double T[3], double alpha, double R1[9], double R2[9], double P1[12], double P2[12],
                        int roi1[4], int roi2[4]);
/* cv::initUndistortRectifyMap(K, 0, R, P, size, CV_32FC1, map1, map2) (wass_stereo.cpp:600-601); maps are
 * [height][width] float32 source coordinates. */
int wass_init_rectify_map(const double K[9], const double R[9], const double P[12], int width, int height,
                          float* map_x, float* map_y);

/* Per-frame resampling on the GPU.  roi == NULL writes the full dw x dh image; otherwise only the
 * roi = {x, y, width, height} window of it is produced (the .clone() crops of wass_stereo.cpp:526-528,606-607
 * fused into the resampler) and dst is roi.width x roi.height, tightly packed. */

/* cv::remap(src, dst, map1, map2, cv::INTER_CUBIC) for CV_8UC1 / CV_32FC1 maps, BORDER_CONSTANT 0
 * (wass_stereo.cpp:603-604): 1/32-pixel coordinate quantisation, 15-bit fixed-point 4x4 weights. */
int wass_remap_cubic(wass_ctx* ctx, const uint8_t* src, int sw, int sh, size_t src_stride, const float* map_x,
                     const float* map_y, int dw, int dh, const int roi[4], uint8_t* dst);
int wass_remap_cubic_dev(wass_ctx* ctx, const uint8_t* d_src, int sw, int sh, size_t src_stride,
                         const float* d_map_x, const float* d_map_y, int dw, int dh, const int roi[4],
                         uint8_t* d_dst);
/* Row f2: cv::undistort(src, dst, K, dist) of wass_prepare (src/wass_prepare/wass_prepare.cpp:268): new camera
 * matrix = K, INTER_LINEAR, BORDER_CONSTANT 0, stripe-wise 1/32-pixel fixed-point maps.  dist = n_dist
 * coefficients in OpenCV order k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]] (n_dist = 4, 5, 8 or 12; the tilt
 * model is not supported).  dst is w x h, tightly packed. */
int wass_undistort(wass_ctx* ctx, const uint8_t* src, int w, int h, size_t src_stride, const double K[9],
                   const double* dist, int n_dist, uint8_t* dst);
int wass_undistort_dev(wass_ctx* ctx, const uint8_t* d_src, int w, int h, size_t src_stride, const double K[9],
                       const double* dist, int n_dist, uint8_t* d_dst);
/* Row f2: cv::CLAHE::apply(src, dst) of wass_prepare (wass_prepare.cpp:257-262; createCLAHE(clip_limit, Size(tiles_x,
 * tiles_y)) at :446-449), CV_8UC1: clipped per-tile histograms, bilinear blend of the four neighbouring look-up tables.
 * dst is w x h, tightly packed. */
int wass_clahe(wass_ctx* ctx, const uint8_t* src, int w, int h, size_t src_stride, double clip_limit, int tiles_x, int tiles_y,
               uint8_t* dst);
int wass_clahe_dev(wass_ctx* ctx, const uint8_t* d_src, int w, int h, size_t src_stride, double clip_limit, int tiles_x, int tiles_y,
                   uint8_t* d_dst);
/* ---- Polarimetric preparation: process_image with do_demosaic of wass_prepare (wass_prepare.cpp:52-85, :103-255) in one pass.
 * mosaic is the u8 picture of a polarising-filter-array camera, rows x cols, macro-pixels  I90 I45 / I135 I0 ; m = rows / 2,
 * n = cols / 2 (an odd last row or column is dropped) and every result is 2m x 2n, tightly packed.  Per pixel: the four quarter
 * pictures as float32, u8 * (1.0f / 255.0f); upscaled x2 as cv::resize INTER_LINEAR does for floats, along x and then along y
 * (weights 0.25 / 0.75; first and last row and column copied); undistorted with the map of the undistort entry above for
 * (K, dist) -- K applies to the 2m x 2n picture -- and the float32 sampler of the remap_linear_f32 entry (its 1024 x 2 x 2 table, the
 * same order of the sum, taps outside the picture 0); mixed so that I0 + I90 = I45 + I135 (k1 = 0.75, k2 = 0.25, left to right);
 * S0 = (((I0 + I45) + I90) + I135) * 0.5f, S1 = I0 - I90, S2 = I45 - I135.  Every float32 product and sum is rounded on its own.
 *   image      u8, always: sat_u8(rint(S0 * 127.0f)), or with hdr != 0 sat_u8(rint(HDR * 255.0f)), HDR = sum(w I) / sum(w) over the
 *              four channels in the order 0, 45, 90, 135, w = float32(exp(double(arg))), arg = (-1.0f * (d * d)) / (2.0f * 0.3f * 0.3f),
 *              d = I - 0.5f; then, with clahe_tiles > 0, the CLAHE entry above with (clahe_clip, clahe_tiles, clahe_tiles) applied
 *   S          float32 [3][2m][2n]
 *   dolp       u8: sat_u8(rint(dolp * 255.0f)), dolp = sqrt(S1 S1 + S2 S2) / S0 in float32
 *   aolp       u8: sat_u8(rint(a * float32(255.0 / 3.1415) + 127.0f)), a = (float32(ang) - 3.1415f) * 0.5f, ang = atan2(S1, S2) in
 *              fp64 plus 2 pi where negative (the reference's cartToPolar is a 0.3 degree approximation; this is the arctangent)
 *   channels   u8 [4][2m][2n]: sat_u8(rint(I * 255.0f)) of the mixed I0, I45, I90, I135
 *   image_f32, aolp_f32   float32: the value of image (before CLAHE) and of aolp before rint and sat_u8
 * sat_u8 clamps to 0 ... 255 and turns NaN into 0; rint rounds half to even.  Only the results named in params->outputs are written
 * (their pointers must not be NULL); image is always written.  ranges = min and max of S0, S1, S2 and dolp, NaN skipped (dolp: NaN
 * unless WASS_PREP_DOLP).  Errors as for the undistort entry; rows or cols below 2: WASS_ERR_INVALID_ARG; 2m or 2n above 32767:
 * WASS_ERR_UNSUPPORTED.  stride is in bytes.  _dev: mosaic and the results are device memory.  Both return after a synchronisation.
 * Written from knowledge of OpenCV 4.5.5 and not pinned against it. */
#define WASS_PREP_STOKES 1
#define WASS_PREP_DOLP 2
#define WASS_PREP_AOLP 4
#define WASS_PREP_CHANNELS 8
#define WASS_PREP_IMAGE_F32 16
#define WASS_PREP_AOLP_F32 32
#define WASS_PREP_ALL 63
typedef struct wass_pol_prep_params {
    int hdr;                /* 0: image = S0 x 127; otherwise the HDR picture x 255 */
    int outputs;            /* WASS_PREP_* bits */
    double clahe_clip;
    int clahe_tiles;        /* 0: no CLAHE */
    int reserved;
} wass_pol_prep_params;
typedef struct wass_pol_prep_out {
    float* S;
    uint8_t* image;
    uint8_t* dolp;
    uint8_t* aolp;
    uint8_t* channels;
    float* image_f32;
    float* aolp_f32;
    float ranges[8];        /* S0 min, S0 max, S1 min, S1 max, S2 min, S2 max, dolp min, dolp max */
} wass_pol_prep_out;
int wass_prepare_pol(wass_ctx* ctx, const uint8_t* mosaic, int cols, int rows, size_t stride, const double K[9], const double* dist,
                     int n_dist, const wass_pol_prep_params* params, wass_pol_prep_out* out);
int wass_prepare_pol_dev(wass_ctx* ctx, const uint8_t* d_mosaic, int cols, int rows, size_t stride, const double K[9],
                         const double* dist, int n_dist, const wass_pol_prep_params* params, wass_pol_prep_out* out);
/* cv::warpPerspective(src, dst, H, Size(dw,dh)) with the default INTER_LINEAR / BORDER_CONSTANT 0
 * (wass_stereo.cpp:515-516); H maps source to destination pixels (it is inverted internally). */
int wass_warp_perspective(wass_ctx* ctx, const uint8_t* src, int sw, int sh, size_t src_stride, const double H[9],
                          int dw, int dh, const int roi[4], uint8_t* dst);
int wass_warp_perspective_dev(wass_ctx* ctx, const uint8_t* d_src, int sw, int sh, size_t src_stride,
                              const double H[9], int dw, int dh, const int roi[4], uint8_t* d_dst);

/* ---- KAZE feature detector (kaze.hip; wass_amd/features.py chains the stages) --------------------------------------------------
 * What FeatureSet::detect asks of cv::KAZE::create(false, false, threshold, n_octaves, n_sublevels): soffset 1.6, sderivatives 1,
 * PM-G2 diffusivity, M-SURF 64 descriptor.  Restated from the published algorithm, not pinned against OpenCV.
 * All planes are h x w float32, contiguous; a stack of levels is `plane_stride` floats apart.  Everything is float32 in the
 * order written here, without contraction, division and square root correctly rounded; every call returns after a
 * synchronisation.  3 <= h, w <= 32768.
 *
 * convert:  dst = (float)src * scale.
 * gauss:    separable, rows then columns, border replicated, acc = acc + tap[j] * v from the first tap to the last (taps: host
 *           pointer, an odd number <= 15).  d_tmp holds the row pass.
 * scharr:   reach s = sigma_size, reflect-101 (s < h, w), norm and wnorm = w * norm given by the caller:
 *             Lx = (norm * d(y-s) + wnorm * d(y)) + norm * d(y+s),  d(r) = src[r][x+s] - src[r][x-s]
 *             Ly = m(y+s) - m(y-s),  m(r) = (norm * src[r][x-s] + wnorm * src[r][x]) + norm * src[r][x+s]
 * hessian:  from the UNSCALED Lx, Ly of scharr: Lxx = scharr_x(Lx) * s^2, Lxy = scharr_y(Lx) * s^2, Lyy = scharr_y(Ly) * s^2,
 *           Ldet = Lxx * Lyy - Lxy * Lxy; then Lx and Ly are multiplied by s in place.  d_lxx, d_lxy, d_lyy may be null.
 * contrast: over the interior pixels m = sqrt(Lx * Lx + Ly * Ly); hmax = the largest; npoints = the moduli that are not 0; hist[300]:
 *           bin floor(300 * (m / hmax)) clamped to 299, of the non-zero ones.  Integer atomics: the same in any launch order.
 *           d_rec: 302 uint32 of device scratch.
 * flow:     1 / (1 + (Lx * Lx + Ly * Ly) / (k * k)).
 * diffuse:  for every tau (host pointer) L <- L + (0.5 * tau) * (((xpos - xneg) + ypos) - yneg) with xpos = (c[E] + c) * (L[E] - L),
 *           xneg = (c + c[W]) * (L - L[W]), ypos = (c[S] + c) * (L[S] - L), yneg = (c + c[N]) * (L - L[N]), a term being 0 where its
 *           neighbour is outside; d_tmp is the other side of the ping-pong, the result ends in d_lt.
 * extrema:  levels 1 .. n_levels-2, interior pixels, v = Ldet > threshold and >= 1e-5, strictly above its 26 neighbours, and
 *           rint(x -+ 3 * esigma[level]) in [0, w), the same for y.  Appends the key (level * h + y) * w + x in any order; *count is
 *           the number found.  More than `cap` returns WASS_KAZE_CAP_REACHED with the first `cap` arrivals in d_keys, valid but
 *           not a defined subset.  d_count: one uint32 of device scratch.
 * refine:   per key Dx = 0.5 (C[x+1] - C[x-1]), Dy, Ds alike (Ds = 0.5 (up - down)); Dxx = (C[x+1] + C[x-1]) - 2 C, Dyy, Dss alike;
 *           Dxy = 0.25 ((C[y+1][x+1] + C[y-1][x-1]) - (C[y-1][x+1] + C[y+1][x-1])), Dxs = 0.25 ((U[x+1] + D[x-1]) - (U[x-1] + D[x+1])),
 *           Dys alike.  [Dxx Dxy Dxs; Dxy Dyy Dys; Dxs Dys Dss] d = -[Dx Dy Ds] by elimination on the 3 x 4 tableau: per column k the
 *           row >= k with the largest |a[r][k]| (the first of equals) is swapped in, f = a[r][k] / a[k][k], a[r][c] = a[r][c] - f * a[k][c]
 *           for c = k+1 .. 3; then d2 = a23 / a22, d1 = (a13 - a12 d2) / a11, d0 = ((a03 - a01 d1) - a02 d2) / a00.
 *           out: n x 5 float32 = x + d0, y + d1, d2, |v|, kept; kept = 0 (x, y unrefined) where a pivot is 0 or some |d| > 1.
 * orientation, descriptors: kp is n x 5 float32 (x, y, size, level, angle), Lx / Ly the scaled stacks.  s = (int)(size / 2 + 0.5).
 *           Orientation: the 109 lattice samples (i outer, j inner, i^2 + j^2 < 36) at ((int)(x + i s + 0.5), (int)(y + j s + 0.5)) inside
 *           the picture, weighted by SURF's gauss25[|i|][|j|]; 42 windows of pi / 3 starting at 0, 0.15, ... (accumulated in float32),
 *           each summed in sample order; the first window with the largest sumX^2 + sumY^2 gives atan2f(sumY, sumX) in [0, 2 pi).
 *           Descriptor: 4 x 4 subregions of 9 x 9 samples, step s, rotated by the angle, bilinear samples (pixels floor and floor + 1, the fraction taken
 *           first, then the indices clamped into the picture),
 *           Gaussian 2.5 s about the subregion, 1.5 about the grid; (sum dx, sum dy, sum |dx|, sum |dy|) per subregion, each summed
 *           in sample order, the 64 values divided by their length.  atan2f, sinf, cosf, expf: bounded, not exact. */
#define WASS_KAZE_MAX_LEVELS 32
#define WASS_KAZE_MAX_CANDIDATES (1 << 20)
#define WASS_KAZE_CAP_REACHED 1
int wass_kaze_scratch_bytes(int h, int w, int n_levels, size_t* bytes);
int wass_kaze_convert_dev(wass_ctx* ctx, const uint8_t* d_src, size_t pitch, int h, int w, float scale, float* d_dst);
int wass_kaze_gauss_dev(wass_ctx* ctx, const float* d_src, int h, int w, const float* taps, int ntaps, float* d_tmp, float* d_dst);
int wass_kaze_scharr_dev(wass_ctx* ctx, const float* d_src, int h, int w, int sigma_size, float norm, float wnorm, float* d_lx, float* d_ly);
int wass_kaze_hessian_dev(wass_ctx* ctx, float* d_lx, float* d_ly, int h, int w, int sigma_size, float norm, float wnorm, float* d_ldet,
                          float* d_lxx, float* d_lxy, float* d_lyy);
int wass_kaze_contrast_dev(wass_ctx* ctx, const float* d_lx, const float* d_ly, int h, int w, uint32_t* d_rec, float* hmax, uint32_t* npoints,
                           uint32_t* hist);
int wass_kaze_flow_dev(wass_ctx* ctx, const float* d_lx, const float* d_ly, int h, int w, float k, float* d_flow);
int wass_kaze_diffuse_dev(wass_ctx* ctx, float* d_lt, float* d_tmp, const float* d_flow, int h, int w, const float* taus, int ntaus);
int wass_kaze_extrema_dev(wass_ctx* ctx, const float* d_ldet, size_t plane_stride, int n_levels, int h, int w, float threshold,
                          const float* esigma, int64_t* d_keys, int cap, uint32_t* d_count, uint32_t* count);
int wass_kaze_refine_dev(wass_ctx* ctx, const float* d_ldet, size_t plane_stride, int n_levels, int h, int w, const int64_t* d_keys, int n,
                         float* d_out);
int wass_kaze_orientation_dev(wass_ctx* ctx, const float* d_kp, int n, const float* d_lx, const float* d_ly, size_t plane_stride, int n_levels,
                              int h, int w, float* d_angle);
int wass_kaze_descriptors_dev(wass_ctx* ctx, const float* d_kp, int n, const float* d_lx, const float* d_ly, size_t plane_stride, int n_levels,
                              int h, int w, float* d_desc);

/* ---- variational refinement of the gridded surface (vref.hip; wass_amd/refinement.py) ------------------------------------------
 * gridding/wassgridsurface/TFVariationalRefinement.py: a half-resolution height field Zc [ny / 2][nx / 2] is moved by Adam so that
 * the two pictures, sampled where the nodes of Z = resize(Zc) project, agree, with a derivative-of-Gaussian smoothness term.
 * Everything is float32 in the order written at the head of vref.hip (projection sums left to right, the 49 taps in row-major
 * order, tfa's bilinear sampler, tf.image.resize with half-pixel centres, Keras's Adam with beta 0.9 / 0.999), without
 * contraction; the gradient is derived by hand and is one sequence of operations per node, so a trajectory does not depend on
 * the launch shape.  The two loss sums are fp64.  Restated from knowledge, not pinned against TensorFlow.
 *
 * Every d_ pointer is device memory, contiguous; every call runs on the context's stream and returns after a synchronisation.
 * create: the set-up is copied into the handle's own allocation (scratch_bytes says how large): d_xb = XX / baseline and
 *   d_yb = YY / baseline [ny][nx] float32, d_mask [ny][nx] float32, the two pictures as float32 [ih][iw]; Rp2c, Tp2c, P0cam,
 *   P1cam are host fp64 and are cast to float32; kernels: host, 2 x 49 float32, the x then the y derivative kernel, row-major.
 *   2 <= ny, nx, ih, iw <= 32768; values that are not finite are refused.
 * sample:   d_I0s, d_I1s [ny][nx] and d_uv [4][ny][nx] = u0, v0, u1, v1 for a full-resolution d_Z.  A node with s_k2 <= 0 or a
 *           coordinate that is not finite in either camera samples 0 in both and adds nothing to the data term or its gradient.
 * zgrad:    the two correlations of d_Z with the kernels, zero padding.
 * loss:     data = mean(((I0s - I1s) / 255)^2), smoothness = mean(Zdx^2 + Zdy^2) over all ny * nx nodes.
 * gradient: d(data + alpha * smoothness) / dZc into d_gC [ny / 2][nx / 2]; d_gZ (may be null): the same with respect to Z.
 * adjoint:  the backward half alone, on planes given by the caller: gZ = d_gd + cS * (the correlations of d_Zdx and d_Zdy with the flipped
 *           kernels), cS = float32(2 alpha / (ny nx)), then d_gC = the adjoint of the resize applied to gZ.  What gradient runs after
 *           its forward half; it lets a test put a single value into one plane and read the footprint.
 * optimize: `iters` Adam steps on d_Zc in place.  d_m, d_v and *step are the optimiser's state, in and out (zeros and 0 to start):
 *           a run continued through them equals one longer run bit for bit.  trace (host, may be null): rows of four doubles
 *           [steps done in this call, data, smoothness, data + alpha * smoothness]: before the first step, after step i (from 0)
 *           where i % report_every == 0, and after the last one; report_every <= 0: the first and the last only.  At most trace_cap
 *           rows, *n_trace written.  The rows are made on the device and read once at the end; no iteration waits for the host.
 *           d_Zout (may be null): resize(Zc) * mask [ny][nx].
 * A Z, Zc, m or v that holds a value that is not finite, iters < 0 and null pointers return WASS_ERR_INVALID_ARG. */
typedef struct wass_vref wass_vref;
int wass_vref_scratch_bytes(int ny, int nx, int ih0, int iw0, int ih1, int iw1, size_t* bytes);
int wass_vref_create(wass_ctx* ctx, int ny, int nx, const float* d_xb, const float* d_yb, const float* d_mask, const double Rp2c[9],
                     const double Tp2c[3], const double P0cam[12], const double P1cam[12], const float* d_I0, int ih0, int iw0,
                     const float* d_I1, int ih1, int iw1, const float* kernels, wass_vref** out);
void wass_vref_destroy(wass_vref* h);
int wass_vref_sample(wass_vref* h, const float* d_Z, float* d_I0s, float* d_I1s, float* d_uv);
int wass_vref_zgrad(wass_vref* h, const float* d_Z, float* d_Zdx, float* d_Zdy);
int wass_vref_loss(wass_vref* h, const float* d_Z, double* data_loss, double* smoothness_loss);
int wass_vref_gradient(wass_vref* h, const float* d_Zc, double alpha, float* d_gC, float* d_gZ);
int wass_vref_adjoint(wass_vref* h, const float* d_Zdx, const float* d_Zdy, const float* d_gd, double alpha, float* d_gC, float* d_gZ);
int wass_vref_optimize(wass_vref* h, float* d_Zc, float* d_m, float* d_v, int64_t* step, int iters, double alpha, double lr, double eps,
                       int report_every, double* trace, int trace_cap, int* n_trace, float* d_Zout);

/* ---- the refinement of a sequence: several frames per launch (vref.hip; refinement.refine_sequence, gridding.grid_sequence) --------
 * The kernels above take their frame from blockIdx.z: mask, pictures, Zc, m, v, the slopes, the gradients, the block partials and
 * the trace rows are per frame; XX / b, YY / b, the cameras, the kernels, the axis tables and Adam's lr_t are shared.  Every value
 * is the same sequence of float32 operations and every frame's fp64 partials are folded on their own in the single run's order, so
 * frame i of a batch equals the single run of frame i bit for bit; the wass_vref_ entries above are a batch of one.
 * A batch handle keeps the shared set-up and room for nb frames (batch_scratch_bytes: what create allocates; needs no GPU; the
 * value for nb = 1 is wass_vref_scratch_bytes') and is loaded again and again, with 1 <= n <= nb frames each time; only the frames
 * of the last load are run, read or reported.  It is not a handle for the single entries above, nor the other way round.
 * load:      d_Zi [n][ny][nx] float32, the gridded surfaces in metres, z up, NaN outside; d_mask [n][ny][nx] float32 or null: a
 *            node is inside where d_mask != 0, without d_mask where d_Zi is not NaN; d_I0 [n][ih0][iw0], d_I1 [n][ih1][iw1] float32.
 *            On the device: zin = inside ? (float)(-(double)Zi / baseline) : 0, then Zc = cv.resize's INTER_LINEAR rule applied to
 *            zin (per axis f = (float)((d + 0.5) * (in / out) - 0.5) from fp64, s = floor(f), f -= s, clamped like OpenCV's; a row
 *            is S[s] * (1 - f) + S[s + 1] * f in float32, rows are combined by the same rule), m = v = 0, step = 0.  A value inside
 *            a frame's mask or in a picture that is not finite refuses the whole load (the message names the first such frame)
 *            and leaves nothing loaded.  A frame whose mask is all zero is no error: it stays at 0 and comes back all NaN.
 * set_state / get_state: Zc, m, v as [n][ny / 2][nx / 2] and the step count, in and out; a run continued through them equals one
 *            longer run bit for bit.
 * optimize:  `iters` Adam steps of every loaded frame.  trace (host, may be null): [n][trace_cap][4], per frame the rows of
 *            wass_vref_optimize; *n_trace: rows written per frame.  Made on the device, read once at the end.
 * result:    d_out [n][ny][nx] = inside ? (float)(-(double)Z * baseline) : NaN with Z = resize(Zc) * mask; d_Z (may be null): Z.
 * Null pointers, n outside 1 .. nb, nb < 1, iters < 0, dimensions outside create's, a call before a load: WASS_ERR_INVALID_ARG. */
int wass_vref_batch_scratch_bytes(int nb, int ny, int nx, int ih0, int iw0, int ih1, int iw1, size_t* bytes);
int wass_vref_batch_create(wass_ctx* ctx, int nb, int ny, int nx, const float* d_xb, const float* d_yb, const double Rp2c[9],
                           const double Tp2c[3], const double P0cam[12], const double P1cam[12], int ih0, int iw0, int ih1, int iw1,
                           const float* kernels, wass_vref** out);
void wass_vref_batch_destroy(wass_vref* h);
int wass_vref_batch_load(wass_vref* h, int n, const float* d_Zi, const float* d_mask, const float* d_I0, const float* d_I1, double baseline);
int wass_vref_batch_set_state(wass_vref* h, const float* d_Zc, const float* d_m, const float* d_v, int64_t step);
int wass_vref_batch_get_state(wass_vref* h, float* d_Zc, float* d_m, float* d_v, int64_t* step);
int wass_vref_batch_optimize(wass_vref* h, int iters, double alpha, double lr, double eps, int report_every, double* trace, int trace_cap,
                             int* n_trace);
int wass_vref_batch_result(wass_vref* h, float* d_out, float* d_Z);

#ifdef __cplusplus
}
#endif
#endif
