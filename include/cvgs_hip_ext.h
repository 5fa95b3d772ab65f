/*
 * cvgs_hip_ext.h -- ENGINE EXTENSIONS of libcvgs_hip.so that have no counterpart in the reference's interface: the device-side
 * descriptor queue (cvgs_queue_*: an opt-in submission path, frozen since round 5), the device-side arrival flags of the sharded
 * batched-crop path (cvgs_exchange_*: BASELINE cfg #5, SURVEY.md 8e option 2) and plane tables built on the device from a detector's
 * device-side boxes (cvgs_plane_tables_from_boxes) and warp tables fitted on the device to its device-side landmarks
 * (cvgs_warp_tables_from_points) or shaped from its boxes (cvgs_warp_tables_from_boxes), device-side box selection (cvgs_boxes_select), the decoding of a network's raw head into its
 * candidates (cvgs_head_decode) and the gather of the kept candidates' landmarks (cvgs_points_gather).  The drop-in boundary -- what replaces
 * fk::executeOperations and fk::CircularTensor (reference include/cvGPUSpeedup.cuh:464-627) -- is include/cvgs_hip.h alone; nothing
 * there depends on this file.  Same conventions: plain C, asynchronous on the given stream, 0 or a negative cvgs_status.
 */
#ifndef CVGS_HIP_EXT_H
#define CVGS_HIP_EXT_H

#include "cvgs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device-side descriptor queue (ABI 4) ---------------------------------------------------------------------
 * The reference submits one kernel per executeOperations call (include/cvGPUSpeedup.cuh:464-473 -> fk::executeOperations:
 * one TransformDPP launch).  On MI355X a 50-crop batch is ~1 us of HBM time behind a ~1.8 us launch/drain boundary, and the
 * waves of ONE launch load, then store, all at the same time.  A queue keeps the call shape -- one submit per
 * frame, same chain descriptor -- and removes the boundary: a resident server grid takes batches from a ring; its
 * workgroups walk from batch to batch without a grid-wide barrier, so batch k+1's loads overlap batch k's stores.
 *   cvgs_queue_create   one queue per device (`device` < 0: the calling thread's current device); `depth` ring slots (0 = 128, at most 256); `idle_us`: the server retires
 *                       itself after this long without work (0 = 200 us) and the next submit starts a new one, so the grid
 *                       never outlives its work; a batch without progress for 250 ms (environment: CVGS_QUEUE_STALL_MS) is reported
 *                       as CVGS_ERR_HIP, not waited for -- every workgroup of the server must be resident, so other kernels of the
 *                       process must not hold the whole chip for longer than that.
 *   cvgs_queue_submit   asynchronous; the chain must be K1's hot shape (batched 8UC3 / 8UC4 -- or 16UC3 / 16UC4 / 16SC3 / 16SC4 -- bilinear resize -> [RGB<->BGR]
 *                       mul, sub, div [-> convertTo CV_16F] -> fp32 / fp16 NCHW / CNHW tensor, host descriptors; a ring slot holds 74 planes, larger batches take
 *                       consecutive slots behind ONE ticket) or the same behind crops of
 *                       NV12 / NV21 / P010 decoder surfaces (CVGS_READ_NV12_RESIZE_LINEAR, 3 channels; letterboxing and default planes
 *                       included): anything else returns CVGS_ERR_UNSUPPORTED and belongs to cvgs_execute.  A queue serves ONE
 *                       of the four kinds (8-bit pixels, 16-bit pixels, NV12 / NV21 surfaces, P010 surfaces) -- its first submit decides, the others are then CVGS_ERR_UNSUPPORTED (each kind
 *                       has its own server grid; create a second queue).  The sources must be complete when submit is
 *                       called (the server is not ordered behind any stream); results are bit-identical to cvgs_execute.
 *   cvgs_queue_wait     host waits for a ticket AND every batch submitted before it (tickets are handed out in submit order; the
 *                       server completes batches in any order -- their tasks are spread over its workers -- so the wait looks at every
 *                       batch up to the ticket that it has not yet seen complete); cvgs_queue_stream_wait makes a HIP stream
 *                       wait for the same set instead: ONE one-wave polling kernel on that stream (k1q_wait; an unsatisfied
 *                       hipStreamWaitValue64 on device memory costs ~1.6 ms here), the
 *                       consumer's kernels enqueued behind it see the tensors.  RELEASE ON FAILURE: the gate kernel of a stream-ordered
 *                       submit and the wait kernel return -- and so release the stream -- when the queue's error word is set or their
 *                       time limit expires (the 10 s gate limit / the stall limit); the tensor may then be incomplete and NOTHING on the
 *                       stream says so.  The failure is reported by the next cvgs_queue_wait / submit / stats call (error word != 0):
 *                       a consumer that must not run on an incomplete tensor checks cvgs_queue_wait(ticket) == CVGS_OK first.
 * Environment: CVGS_QUEUE_G = worker workgroups (default 2 per CU - 1 for 8-bit pixel crops, 3 per CU - 1 for the other kinds; the flags' bits 16..27 say the same per queue),
 * CVGS_QUEUE_STALL_MS = the stall watchdog, CVGS_QUEUE_DEBUG=1 = a state dump when it fires (=2: gate timestamps for tools/probes).  Frozen since round 5: no new kinds, no new knobs.
 * Submits from several host threads are serialised by a mutex (tickets are handed out in submit order).  cvgs_queue_destroy
 * waits (at most 2 s) for the batches in flight, then retires the server.  Whether the host writes the ring straight into device
 * memory is decided without a fault (large-BAR attribute + /proc/self/maps + a read-back; flags bit 0 asks for the staged ring).
 * RUNTIME NOTE: while a server grid is alive, kernels of every stream whose hardware queue shares the server queue's command-processor
 * pipe dispatch at ~27 us each instead of ~3.4 us (measured: one stream in four on the default runtime's 4 hardware queues, none with
 * GPU_MAX_HW_QUEUES <= 3; tools/probes/server_vs_streams.py).  Processes that keep a queue alive beside other streams should set
 * GPU_MAX_HW_QUEUES=3 before the HIP runtime initialises; the server retires idle_us after its last batch.
 * No reference counterpart.                                                                                           */
typedef struct cvgs_queue_s* cvgs_queue_t;
int cvgs_queue_create(cvgs_queue_t* out, int32_t device, int32_t depth, double idle_us, uint32_t flags);
int cvgs_queue_submit(cvgs_queue_t q, const cvgs_chain_desc* chain, uint64_t* ticket);
/* n submits in one call (a serving loop's burst); *last_ticket = the ticket of chains[n-1] */
int cvgs_queue_submit_many(cvgs_queue_t q, const cvgs_chain_desc* const* chains, int32_t n, uint64_t* last_ticket);
/* Stream-ordered submit (ABI 5) -- the reference's contract on the queue: cvGS::executeOperations(stream, iops...) is "asynchronous on
 * the given stream" (include/cvGPUSpeedup.cuh:464-473; cv::cuda::StreamAccessor::getStream at :466).  The batch is ordered BEHIND
 * everything already enqueued on `stream` (the decoder / kernel that writes the frame need not be synchronised with the host) and,
 * unless CVGS_QUEUE_SUBMIT_DEFER_WAIT, everything enqueued on `stream` AFTER the call is ordered behind the batch's tensor.  Cost: ONE
 * one-wave kernel on `stream` per call (it opens the batch's gate in the ring when the stream gets there, then holds the stream on the
 * batch's completion word); no host synchronisation, no event, no second stream operation.  Workers that draw a task of a batch whose
 * gate is still closed wait there; other batches proceed.  A gate that stays closed for 10 s is reported
 * as an error (word 3), not waited for.
 *   CVGS_QUEUE_SUBMIT_DEFER_WAIT  the stream is NOT held: the caller orders the consumer itself with cvgs_queue_stream_wait(q, ticket,
 *                                 stream) -- several batches of ONE stream can then be in flight at once (a strictly ordered stream has
 *                                 one, because the next gate sits behind the previous wait).  Until that wait the batch's SOURCES are
 *                                 in flight too: work enqueued on the stream behind the call runs concurrently with the batch and must
 *                                 not rewrite them (a strictly ordered call protects both sides).
 *   CVGS_QUEUE_SUBMIT_HYBRID      latency policy ("never slower than without a queue"): stream order costs one launch per gate, so a
 *                                 gate in front of fewer than 8 chains (CVGS_QUEUE_SUBMIT_MIN_GROUP(n) changes the 8) never beats
 *                                 launching them -- such calls, a batch nothing in flight could overlap with, and any chain the
 *                                 server does not take are launched DIRECTLY on `stream` as cvgs_execute would (*ticket =
 *                                 CVGS_QUEUE_TICKET_DIRECT).  Measured: a lone strict stream 14-16 us per batch on the server against
 *                                 8-9 us as launches; ticks of 16 frames (cvgs_queue_submit_many_on) 2.5 us per frame against 8.9.
 * Not capturable (the ring is written at submit time): CVGS_ERR_UNSUPPORTED on a capturing stream (with HYBRID: the direct launch is
 * captured instead).  At most 74 planes per call.                                                                          */
#define CVGS_QUEUE_SUBMIT_DEFER_WAIT 1u
#define CVGS_QUEUE_SUBMIT_HYBRID 2u
#define CVGS_QUEUE_SUBMIT_MIN_GROUP(n) (((uint32_t)(n) & 0xffu) << 8) /* with HYBRID: the smallest group the server takes (0 = 8) */
#define CVGS_QUEUE_TICKET_DIRECT (~(uint64_t)0)
int cvgs_queue_submit_on(cvgs_queue_t q, const cvgs_chain_desc* chain, cvgs_stream_t stream, uint32_t flags, uint64_t* ticket);
/* n chains (<= CVGS_QUEUE_MAX_GROUP) behind ONE gate kernel: the pictures of one tick -- several cameras' frames written by the work in
 * front of the call, several crop lists of one frame -- are ordered behind `stream` together, overlap on the server, and (unless
 * DEFER_WAIT) the stream is held until ALL of them are complete: one launch per tick instead of one per chain.  The stream-ordered
 * counterpart of cvgs_execute_many / cvgs_queue_submit_many.  A wait on *last_ticket covers the group.  The chains of a group run
 * CONCURRENTLY on the server, so they must be independent -- no chain may write what another chain of the group reads or writes (checked
 * for tensor targets against each other and against host-described sources, as cvgs_execute_many does; sources in caller-owned device
 * tables cannot be checked): a dependent group is launched one by one, in order, under HYBRID and is CVGS_ERR_UNSUPPORTED without it.
 * A caller stream created at the HIGHEST stream priority (the server's own) may share the server's hardware queue, where its gate kernel
 * could never start: such streams are not taken by the server (HYBRID: direct launches; otherwise CVGS_ERR_UNSUPPORTED).  With HYBRID, groups below the
 * minimum and chains the server does not take are launched one by one on the stream, in order -- and a STRICTLY ordered group (no
 * DEFER_WAIT, no explicit MIN_GROUP) is ONE multi-chain launch on the stream (cvgs_execute_many; *last_ticket = CVGS_QUEUE_TICKET_DIRECT):
 * the stream is held until the group is complete either way, and measured (ticks of 16 frames, a producer on the stream) the launch
 * serves a frame in 2.4-3.0 us where gate + server take 2.7-3.4, with nothing resident beside the consumer.  The server keeps what it is
 * better at: deferred waits (2.4-2.5 us per frame on ONE stream) and host tickets (cvgs_queue_submit, 2.15).               */
#define CVGS_QUEUE_MAX_GROUP 64
int cvgs_queue_submit_many_on(cvgs_queue_t q, const cvgs_chain_desc* const* chains, int32_t n, cvgs_stream_t stream, uint32_t flags, uint64_t* last_ticket);
/* After a wait / submit has reported CVGS_ERR_HIP because the server's watchdog fired (another kernel held the chip beyond
 * CVGS_QUEUE_STALL_MS, a gate never opened): waits for the failed server to leave, declares the batches that were in flight lost
 * (*lost = how many; waits on their tickets return CVGS_ERR_HIP, streams waiting for them are released, their tensors may be
 * incomplete), resets the protocol state and clears the error -- the next submit starts a fresh server.  A no-op on a healthy queue. */
int cvgs_queue_recover(cvgs_queue_t q, uint64_t* lost);
int cvgs_queue_wait(cvgs_queue_t q, uint64_t ticket, double timeout_s);
int cvgs_queue_stream_wait(cvgs_queue_t q, uint64_t ticket, cvgs_stream_t stream);
/* out[8]: submitted, completed, server launches, feeder rounds and lifetime (100 MHz ticks) of the last retired server,
 * worker workgroups, ring slots, error word */
int cvgs_queue_stats(cvgs_queue_t q, uint64_t* out8);
/* the hipStream_t the server grid is launched on (for HIP events / profilers; do not enqueue work behind a live server) */
cvgs_stream_t cvgs_queue_stream(cvgs_queue_t q);
/* out[16], of the last RETIRED server, 100 MHz ticks / counts: feeder {rounds with copies, slots, 0, 0 (reserved)},
 * monitor {scans, scan ticks, ring waits of the host, batches complete behind an incomplete oldest one (mean)}, worker 0 {tasks, find ticks, rows ticks, drain
 * ticks, idle polls}, host ns per submit spent waiting for a ring slot, stream-ordered submits taken by the server | launched directly << 32, gate trace address (probes) */
int cvgs_queue_profile(cvgs_queue_t q, uint64_t* out16);
int cvgs_queue_destroy(cvgs_queue_t q);

/* ---- device-side arrival flags for the sharded batched-crop path (ABI 4; BASELINE cfg #5, SURVEY.md 8e option 2) ----------
 * With the P2P fused write (cvgs_write_desc.mirrors) every rank's K1 launch stores its rows of the [N,C,H,W] tensor into every
 * peer's copy; what remains of the exchange is knowing when all rows of a step have landed.  These two calls keep that on the
 * device: flags are 8-byte words the ranks place in their IPC-shared allocations (include/cvgs_rccl.h: cvgs_ipc_*), one word per
 * source rank, at least 128 bytes apart.
 *   cvgs_exchange_signal  enqueue behind the step's launch: stores `value` (the step number, monotonic) into the n given words --
 *                         this rank's word in each peer's flag block (pointers valid in THIS process).  The kernel boundary in
 *                         front of it makes the step's rows visible before the flags.
 *   cvgs_exchange_wait    the stream waits until each of the n given words (this rank's own flag block: one word per peer)
 *                         is >= `value`; after `timeout_ms` (0 = 2000) it gives up, stores {1, index of a flag that was behind}
 *                         into err_words[0..1] (device or pinned memory, may be NULL) and lets the stream continue -- a lost
 *                         peer is reported, never waited for; while err_words[0] is non-zero every later wait / step behind the same
 *                         error words returns at once (ONE timeout per lost peer, not one per step; clear the words to re-arm).  n <= 16.
 * `step_counter` (device memory, 8 bytes, zero-initialised by the caller; NULL = use `value`): the step number then lives on the
 * device -- signal advances *step_counter and publishes the new count, wait waits for *step_counter - lag (and for nothing while
 * the count is <= lag) -- so that a whole sequence of steps can be captured into ONE HIP graph and replayed (a captured constant
 * would repeat).  With n == 0 and a counter, cvgs_exchange_signal still advances it; cvgs_exchange_step with n == 0 enqueues NOTHING and
 * leaves the counter alone (one rank has nobody to tell and nothing to wait for -- the two differ on purpose).
 * No collective and no host round trip per step.  No reference counterpart (the reference is single-GPU).                 */
int cvgs_exchange_signal(void* const* peer_flag_words, int32_t n, uint64_t value, uint64_t* step_counter, cvgs_stream_t stream);
int cvgs_exchange_wait(const void* const* own_flag_words, int32_t n, uint64_t value, const uint64_t* step_counter, uint64_t lag, double timeout_ms,
                       void* err_words, cvgs_stream_t stream);
/* signal + lagged wait as ONE launch per step (what a steady loop enqueues behind each K1): advances *step_counter, publishes it
 * into peer_flag_words[0..n), then waits until own_flag_words[0..n) have reached the count - lag.  n == 0 (one rank): nothing is
 * enqueued.  About one kernel boundary (~2 us) per step, against >= 20 us of link time per step on 8 GPUs.                      */
int cvgs_exchange_step(void* const* peer_flag_words, const void* const* own_flag_words, int32_t n, uint64_t* step_counter, uint64_t lag,
                       double timeout_ms, void* err_words, cvgs_stream_t stream);

/* ---- device-built plane tables: crops from a detector's device-side boxes ------------------------------------------------------
 * The second stage of a detection pipeline reads boxes that a network has just written on the same GPU.  Every other way to describe a
 * crop (cvgs_image2d arrays, cvgs_plane_table_build) goes through the host: copy the boxes back, synchronise, build, launch again.
 * cvgs_plane_tables_from_boxes enqueues ONE small kernel on `stream` that writes the device plane tables of up to CVGS_MAX_CHAINS
 * frames from boxes in device memory (grid y = frame, one work-item per box; the n descriptors travel in the kernel arguments).
 * Nothing is allocated, staged or synchronised, and the launch can be captured into a HIP graph between the producer of the boxes and
 * the chains that read the tables.  Its cost has not been timed.
 *
 * Boxes are clamped into the frame; `xb / yb` of CVGS_BOX_XYXY_F32 are exclusive edges in pixel coordinates:
 *   XYXY_F32  four floats (xa, ya, xb, yb): l = (int)floorf(fminf(fmaxf(xa, 0), W)), r = (int)ceilf(fminf(fmaxf(xb, 0), W)), t / b the
 *             same with H.  The clamp comes first, so +-inf and values beyond the int range are fine; a NaN in any slot makes the box invalid.
 *   XYWH_I32  four int32 (x, y, w, h): l = clamp(x, 0, W), r = clamp((int64)x + w, 0, W), t / b the same; w <= 0 or h <= 0: invalid.
 * 4:2:0 frames (CVGS_READ_NV12_RESIZE_LINEAR, NV12 / NV21): l and t are then rounded DOWN to even, r and b UP to even and clamped again, so
 * that every view is one the host lowering accepts (even origin, even size).  The frame's width, height and step must be even.
 * A box is VALID iff r > l && b > t after that.  `count` (device int32, or NULL = max_boxes) is clamped to [0, max_boxes]; entries at or
 * beyond it are invalid boxes.
 *   valid box    table_out[i] = exactly what cvgs_plane_table_build writes for the view data = frame.data + t*step + l*elemSize, width =
 *                r - l, height = b - t, step = the frame's (4:2:0: uv_offset = frame's chroma offset + (t/2)*step + l - (t*step + l)),
 *                with dst_width / dst_height / aspect_ratio: the same bytes (scale factors included: same fp32 / fp64 operations, same
 *                source text on both sides).
 *   invalid box  a plane that yields the chain's background value in every pixel and reads only bytes of the frame: the frame's own
 *                data / width / height / step (4:2:0: its chroma offset, uv_offset or height * step), fx = fy = 1, and the EMPTY
 *                destination window x1 = y1 = 0, x2 = y2 = -1 -- every kernel that takes a device table sends pixels outside the
 *                window through the background path, as it does for aspect-ratio padding.
 *   rects_out    optional, device int32[max_boxes][4]: (l, t, r - l, b - t) of a valid box, (0, 0, 0, 0) of an invalid one -- maps the
 *                consumer's results back to frame coordinates.
 * USING THE TABLE: a chain passes table_out as read.src with CVGS_READ_FLAG_TABLE_ON_DEVICE, batch = used_planes = max_boxes (validity is
 * per plane, inside the table; used_planes only describes a tail), the same kind / src_type / yuv_layout / dst size / aspect ratio.
 * INDEPENDENCE (cvgs_execute_many): such a chain states read.table_src_lo / table_src_hi = the byte range of the WHOLE frame, which is
 * cvgs_plane_table_hull of the one whole-frame view (chroma rows included).  Every box is clamped into the frame, whatever the device
 * writes, so that range holds every byte the table's planes can read: exact enough, and always safe.
 * Validation happens completely on the host before the first HIP call (a machine without a GPU can test it): null pointers, struct_size,
 * flags, n outside 1..CVGS_MAX_CHAINS, max_boxes outside 1..65535, misaligned pointers (table_out: 8 bytes; boxes / count / rects_out: 4),
 * the frame checks of the host lowering -> CVGS_ERR_INVALID; per-pixel (CVGS_READ_PIXEL / CVGS_READ_NV12) and warp read kinds, YUV
 * layouts other than NV12 / NV21 (device tables carry no layout tag), frames or targets beyond CVGS_MAX_DIM, targets for which
 * dst_height * frame.width or dst_width * frame.height exceeds 2^30 -> CVGS_ERR_UNSUPPORTED.  The tables and rectangle buffers of one call
 * must not overlap.  No reference counterpart.                                                                                      */
typedef enum cvgs_box_format { CVGS_BOX_XYXY_F32 = 0, CVGS_BOX_XYWH_I32 = 1 } cvgs_box_format;
typedef struct cvgs_box_table_desc {
    uint32_t struct_size, flags;      /* sizeof(cvgs_box_table_desc); flags: must be 0 */
    cvgs_image2d frame;               /* the WHOLE frame / surface (device pointer) */
    int32_t read_kind;                /* CVGS_READ_RESIZE_LINEAR or CVGS_READ_NV12_RESIZE_LINEAR */
    int32_t src_type, yuv_layout;     /* NV12 kind: CVGS_YUV_NV12 / NV21 only (what device tables serve today) */
    int32_t dst_width, dst_height, aspect_ratio;
    int32_t box_format, max_boxes;    /* cvgs_box_format; 1..65535 */
    const void* boxes;                /* device: max_boxes x 4 floats / int32 */
    const int32_t* count;             /* device, or NULL */
    void* table_out;                  /* device, cvgs_plane_table_bytes(max_boxes) */
    int32_t* rects_out;               /* device, or NULL */
} cvgs_box_table_desc;
int cvgs_plane_tables_from_boxes(const cvgs_box_table_desc* descs, int32_t n, cvgs_stream_t stream);

/* ---- device-built warp tables: aligned crops from a detector's device-side landmarks ---------------------------------------------------
 * cvGS::warp is the other second-stage read: align N faces to a 5-point template, rectify N oriented detections, hand them to the
 * network.  cvgs_warp_tables_from_points enqueues ONE small kernel on `stream` (csrc/k_points.hip) that fits the transforms where the
 * landmarks are and writes the device warp tables of up to 16 frames (grid y = frame, one work-item per item; descriptors and templates
 * travel in the kernel arguments).  Nothing is allocated, staged or synchronised; the launch can be captured between the producer of the
 * points and the chains that read the tables.  Its cost has not been timed.
 *
 * A table entry is 64 bytes: {data, width, height, step} of the frame, float m[9] (row-major 3x3, DESTINATION -> SOURCE: what the warp
 * kernels consume), {dst_width, dst_height}.  Coordinates follow the warp kernels' convention, which is cv::warpAffine's: integer
 * coordinates are pixel centres.  The fit is computed in double, in one written order shared by host and device (csrc/cvgs_geometry.h:
 * warp_fit; sums over the points in index order, no sqrt / sin / cos, -ffp-contract=off, correctly rounded division) and narrowed to float
 * at the end, so the device-built table equals cvgs_warp_table_build_host byte for byte.
 *   CVGS_WARP_FIT_SIMILARITY  n_points = 2..16 landmarks p_i (frame pixels) and the template q_i (destination pixels): the least-squares
 *                             NON-REFLECTIVE similarity taking p -> q (the forward fit of skimage's SimilarityTransform / insightface's
 *                             estimate_norm), in closed form -- with centred pc, qc and den = sum |pc|^2: a = sum pc.qc / den,
 *                             b = sum (pc.x qc.y - pc.y qc.x) / den, t = mean(q) - [a -b; b a] mean(p) -- then inverted in closed form
 *                             (n = a^2 + b^2).  Row 2 is 0 0 1.
 *   CVGS_WARP_FIT_AFFINE3     exactly three points and a three-point template (three corners of an oriented box): the exact affine with
 *                             M (q_j, 1) = p_j, by Cramer's rule on the template's edge vectors.  Row 2 is 0 0 1.
 * An item is INVALID when any of its 2 * n_points coordinates is not finite; (similarity) den == 0, n == 0 or either is not finite; any of
 * the six narrowed floats is not finite; or its index is at or beyond `count` (device int32, or NULL = max_items; clamped to
 * [0, max_items]).  An invalid item gets m = {0,0,-1, 0,0,-1, 0,0,1}: every destination pixel maps to (-1, -1), outside the source, which
 * every warp kernel renders as 0 followed by the chain's program -- the plane reads nothing.  valid_out (optional, device
 * int32[max_items]) receives 1 / 0.
 * WHY THE TABLE IS SAFE WHATEVER THE DEVICE BUFFER HOLDS: the warp kernels test 0 <= sx < width && 0 <= sy < height before any tap, and
 * width / height / step / data of every entry are the frame the HOST validated here; NaN, +-inf and huge matrices all fail that test and
 * give 0.  The points only ever decide WHERE inside the frame a plane reads.
 * USING THE TABLE: a warp chain (CVGS_READ_WARP_AFFINE / _PERSPECTIVE) passes table_out as read.src with CVGS_READ_FLAG_TABLE_ON_DEVICE,
 * batch = max_items (<= 65535), used_planes <= batch (planes beyond it take the default value), dst_width / dst_height = the builder's,
 * warp_matrices == NULL and warp_dst_sizes == NULL (either non-null: CVGS_ERR_INVALID).  The launch reads the caller's table where a
 * host-described batch beyond the inline limit reads an uploaded copy: nothing is staged, and cvgs_kernel_name gives the names of
 * host-described chains of the same shape (a CV_64F program: the table variant, which host-described batches of more than 8 planes get).
 * CV_64F sources are served through host descriptors only.  cvgs_execute_many fuses independent chains of ONE shape over such tables --
 * 8UC3 / 8UC4 frames, one target size, a cast-free program, planar fp32 / fp16 / bf16 tensors -- into ONE launch (the warp tick: grid
 * z = chain, bit-identical to one cvgs_execute per chain; the chains state the frame's byte range, read.table_src_lo / _hi, or vouch); the
 * same holds for host-described warp chains of at most 256 planes in all, whose descriptors travel in the kernel arguments.  Everything
 * else runs one by one, in order, and cvgs_last_error() says why ("not fused: ...").  The descriptor
 * queue and cvgs_circular_update refuse them (CVGS_ERR_UNSUPPORTED, before anything is enqueued).  The chain may state
 * read.table_src_lo / _hi = the whole frame's byte range.
 * Validation happens completely on the host before the first HIP call: null pointers, struct_size, flags, n outside 1..16, max_items
 * outside 1..65535, misaligned pointers (table_out: 8 bytes; points / count / valid_out: 4), n_points outside the fit's range, non-finite
 * template entries, a similarity template whose points all coincide, an AFFINE3 template of zero area, a non-positive target, a frame
 * that the host lowering would refuse, output buffers of one call that overlap -> CVGS_ERR_INVALID; non-warp read kinds, frames or
 * targets beyond CVGS_MAX_DIM, CV_64F sources -> CVGS_ERR_UNSUPPORTED.
 *   cvgs_warp_table_build_host  the same descriptor with HOST `points`, `count` and (optional) `valid_out`; desc->table_out is ignored and
 *                               the table goes to table_out_host.  Runs the shared fit on the CPU and writes the bytes the kernel must
 *                               write; makes no HIP call.
 * No reference counterpart.                                                                                                          */
typedef enum cvgs_warp_fit { CVGS_WARP_FIT_SIMILARITY = 0, CVGS_WARP_FIT_AFFINE3 = 1 } cvgs_warp_fit;
#define CVGS_WARP_MAX_POINTS 16
#define CVGS_WARP_MAX_FRAMES 16
typedef struct cvgs_warp_table_desc {
    uint32_t struct_size, flags;      /* sizeof(cvgs_warp_table_desc); flags: must be 0 */
    cvgs_image2d frame;               /* the WHOLE frame (device pointer) */
    int32_t src_type;
    int32_t read_kind;                /* CVGS_READ_WARP_AFFINE or CVGS_READ_WARP_PERSPECTIVE */
    int32_t dst_width, dst_height;
    int32_t fit, n_points;            /* cvgs_warp_fit; SIMILARITY: 2..16, AFFINE3: 3 */
    float tmpl[CVGS_WARP_MAX_POINTS][2]; /* template points (x, y) in destination pixels; entries beyond n_points are ignored */
    int32_t max_items, reserved;      /* 1..65535; 0 */
    const float* points;              /* device: float32 [max_items][n_points][2] (x, y) in frame pixels */
    const int32_t* count;             /* device, or NULL */
    void* table_out;                  /* device, cvgs_warp_table_bytes(max_items) */
    int32_t* valid_out;               /* device, or NULL */
} cvgs_warp_table_desc;
size_t cvgs_warp_table_bytes(int32_t planes);
int cvgs_warp_tables_from_points(const cvgs_warp_table_desc* descs, int32_t n, cvgs_stream_t stream);
int cvgs_warp_table_build_host(const cvgs_warp_table_desc* desc, void* table_out_host);

/* ---- device-built warp tables: context crops from a detector's device-side boxes ---------------------------------------------------------
 * The read top-down pose, ReID and attribute networks are trained on: grow the detector's box by a context factor, grow its shorter side
 * to the network's aspect ratio, and sample that rectangle EVEN WHERE IT LEAVES THE FRAME, filling with 0.  The clamped crop
 * (cvgs_plane_tables_from_boxes) has no margin and squeezes a box at the frame's edge; the warp kernels already render 0 outside the
 * source.  cvgs_warp_tables_from_boxes enqueues ONE small kernel on `stream` (csrc/k_boxwarp.hip) that turns the boxes of up to
 * CVGS_WARP_MAX_FRAMES frames into device warp tables (grid y = frame, one work-item per item; the descriptors travel in the kernel
 * arguments).  Nothing is allocated, staged or synchronised; the launch can be captured between the producer of the boxes (`boxes` /
 * `count` are exactly cvgs_boxes_select's boxes_out / count_out) and the chains that read the tables.  Its cost: see README.md.
 *
 * THE CONTRACT.  One text for the kernel and for cvgs_warp_table_from_boxes_host (csrc/cvgs_geometry.h: box_warp_fit).  Per item,
 * everything in double, in this order, one rounding per operation, no fma (-ffp-contract=off), correctly rounded division, narrowed to
 * float at the end, as the landmark fit does:
 *   1. live = clamp(count ? *count : max_items, 0, max_items); item i >= live is invalid.  The four floats (xa, ya, xb, yb) of a live item --
 *      EDGE coordinates in frame pixels, xb / yb exclusive -- are widened to double; any non-finite value makes the item invalid.
 *   2. w = xb - xa; h = yb - ya; invalid unless w > 0 && h > 0.  cx = (xa + xb) * 0.5; cy = (ya + yb) * 0.5.
 *   3. w1 = w * scale[0]; w1 = w1 + pad[0]; h1 = h * scale[1]; h1 = h1 + pad[1] (the descriptor's floats widened).
 *   4. CVGS_BOX_SHAPE_EXPAND only: t1 = w1 * (double)dst_height; t2 = h1 * (double)dst_width; if t1 > t2: h1 = t1 / (double)dst_width;
 *      else if t2 > t1: w1 = t2 / (double)dst_height; equal: unchanged.  The shorter side grows; no rounded ratio of the target's sides
 *      is ever formed.  CVGS_BOX_SHAPE_STRETCH samples the rectangle of step 3 as it is.
 *   5. Integer coordinates are pixel centres on both sides (the warp kernels' convention): destination centre u is the edge coordinate
 *      u + 0.5.  m0 = w1 / (double)dst_width; m4 = h1 / (double)dst_height;
 *      m2 = (cx - w1 * 0.5) + (m0 * 0.5 - 0.5); m5 = (cy - h1 * 0.5) + (m4 * 0.5 - 0.5); m1 = m3 = 0.
 *   6. m0, m2, m4, m5 are narrowed to float; any of them not finite: the item is invalid.  A valid entry is the frame's {data, width,
 *      height, step}, m = {m0, 0, m2, 0, m4, m5, 0, 0, 1}, {dst_width, dst_height} (the same entry for both read kinds); an invalid one
 *      carries the landmark builder's invalid matrix {0,0,-1, 0,0,-1, 0,0,1}: the plane reads nothing.
 *   7. boxes_out[i] (optional, device float[max_items][4]): the shaped rectangle in frame EDGE coordinates, NOT clamped, each value
 *      narrowed from double: (float)(cx - w1*0.5), (float)(cy - h1*0.5), (float)(cx + w1*0.5), (float)(cy + h1*0.5); (0,0,0,0) for an
 *      invalid item.  It maps second-stage results back to the frame, and is by construction a valid `boxes` of a CVGS_BOX_XYXY_F32
 *      cvgs_box_table_desc (that call clamps: K1 crops gain the margin too).
 *   8. valid_out[i] (optional, device int32[max_items]) = 1 / 0.  Every output element is written on every call.
 * WHY THE TABLE IS SAFE WHATEVER THE DEVICE BUFFER HOLDS: as for the landmark builder -- every entry's frame is the one the HOST validated
 * here, and the matrix only decides where inside it a plane reads (the warp kernels test 0 <= sx < width && 0 <= sy < height before any tap).
 * USING THE TABLE: exactly as a table of cvgs_warp_tables_from_points (above), fused warp tick included.
 * Validation happens completely on the host before the first HIP call: null descriptors or required pointers, struct_size, flags, n
 * outside 1..16, max_items outside 1..65535, a bad shape, scale not finite or <= 0, pad not finite or < 0, a non-positive target,
 * misaligned pointers (table_out: 8 bytes; boxes / count / boxes_out / valid_out: 4), a frame that the host lowering would refuse, output
 * buffers of one call that overlap -> CVGS_ERR_INVALID; non-warp read kinds, CV_64F sources, frames or targets beyond CVGS_MAX_DIM ->
 * CVGS_ERR_UNSUPPORTED.
 *   cvgs_warp_table_from_boxes_host  the same descriptor with HOST `boxes` and `count`; desc's output pointers are ignored and the outputs
 *                                    go to table_out_host (required), boxes_out_host and valid_out_host (either may be NULL).  Runs the
 *                                    shared text on the CPU and writes the bytes the kernel must write; makes no HIP call.
 * Rotated boxes, flips, YUV and CV_64F sources and other box formats are not served.  No reference counterpart.                      */
typedef enum cvgs_box_shape { CVGS_BOX_SHAPE_STRETCH = 0, CVGS_BOX_SHAPE_EXPAND = 1 } cvgs_box_shape;
typedef struct cvgs_box_warp_desc {
    uint32_t struct_size, flags;      /* sizeof(cvgs_box_warp_desc); flags: must be 0 */
    cvgs_image2d frame;               /* the WHOLE frame (device pointer) */
    int32_t src_type;
    int32_t read_kind;                /* CVGS_READ_WARP_AFFINE or CVGS_READ_WARP_PERSPECTIVE */
    int32_t dst_width, dst_height;
    int32_t shape, max_items;         /* cvgs_box_shape; 1..65535 */
    float scale[2], pad[2];           /* context factor per axis (x, y): finite, > 0; pixels added per axis: finite, >= 0 */
    const float* boxes;               /* device: float32 [max_items][4] (xa, ya, xb, yb), edge coordinates in frame pixels */
    const int32_t* count;             /* device, or NULL */
    void* table_out;                  /* device, cvgs_warp_table_bytes(max_items) */
    float* boxes_out;                 /* device float32 [max_items][4], or NULL */
    int32_t* valid_out;               /* device, or NULL */
} cvgs_box_warp_desc;
int cvgs_warp_tables_from_boxes(const cvgs_box_warp_desc* descs, int32_t n, cvgs_stream_t stream); /* n = 1..CVGS_WARP_MAX_FRAMES frames, one call */
int cvgs_warp_table_from_boxes_host(const cvgs_box_warp_desc* desc, void* table_out_host, float* boxes_out_host, int32_t* valid_out_host);

/* ---- device-side box selection: score threshold, top-K, greedy NMS ---------------------------------------------------------------------
 * What sits between a detector and cvgs_plane_tables_from_boxes.  A detector emits thousands of scored candidates, usually in the
 * coordinates of its letterboxed input; the final detections are the few that pass a score threshold and survive non-maximum
 * suppression, in frame coordinates.  cvgs_boxes_select enqueues TWO small kernels on `stream` (csrc/k_select.hip: rank, then suppress)
 * for up to 16 frames and nothing else: no allocation, no staging, no copy, no synchronisation, so the call can be captured between the
 * detector and the table builder.  boxes_out / count_out are by construction a valid boxes / count pair of a CVGS_BOX_XYXY_F32
 * cvgs_box_table_desc with max_boxes = max_out.  Its cost: see README.md.
 *
 * THE CONTRACT.  Arithmetic is strict fp32 (-ffp-contract=off), every operation rounded once, in the order written here; the text is
 * ONE spelling for the kernels and for cvgs_boxes_select_host (csrc/cvgs_geometry.h: select_prepare, select_precedes,
 * select_suppresses), so the device writes the host entry's bytes.  There is no division and no sort whose tie order could differ.
 * Candidate i of a frame reads boxes[i * box_stride + 0..3], scores[i * score_stride] and (if given) classes[i * class_stride]: a
 * [N, 4 + 1 + C] detector head is read in place, and the three pointers may point into one tensor.  Per frame:
 *   1. live = clamp(count ? *count : max_candidates, 0, max_candidates).
 *   2. Candidate i < live is a MEMBER iff its score is not NaN, score >= score_threshold, and none of its four coordinates is NaN.
 *   3. To XYXY.  CVGS_CAND_XYXY_F32: (xa, ya, xb, yb) as read.  CVGS_CAND_CXCYWH_F32 (cx, cy, w, h): hw = w * 0.5f; xa = cx - hw;
 *      xb = cx + hw; hh = h * 0.5f; ya = cy - hh; yb = cy + hh.
 *   4. To frame coordinates with xform = (sx, sy, ox, oy): xa = xa * sx; xa = xa + ox (two roundings, no fma); the same for xb, and
 *      for ya and yb with sy, oy.
 *   5. Clamp: xa = fminf(fmaxf(xa, 0.0f), (float)W), the same for xb, and with H for ya and yb -- spelled v > 0.0f ? v : 0.0f, then
 *      v < e ? v : e, which pins the two cases fmaxf leaves open: -0.0f, and a NaN formed by inf - inf in step 3, both give +0.0f.
 *      A candidate stays a member iff xb > xa && yb > ya.
 *   6. Members are ordered by score descending, equal scores (-0.0f == 0.0f) by lower index first.  The first min(members, pre_nms_k)
 *      form the WORKING LIST.
 *   7. Greedy walk of the working list in that order.  A candidate is KEPT iff no earlier kept candidate suppresses it; with `classes`,
 *      only earlier kept candidates of the same class value count.  j suppresses i iff
 *        iw = fminf(xb_i, xb_j) - fmaxf(xa_i, xa_j), iw > 0.0f;   ih = fminf(yb_i, yb_j) - fmaxf(ya_i, ya_j), ih > 0.0f;
 *        inter = iw * ih;   area = (xb - xa) * (yb - ya) for i and for j;   uni = (area_i + area_j) - inter;
 *        inter > iou_threshold * uni.
 *      The walk stops once max_out candidates are kept.
 *   8. EVERY output element is written on every call: boxes_out[k] = the four clamped floats of the k-th kept candidate for k < kept,
 *      (0, 0, 0, 0) beyond (cvgs_plane_tables_from_boxes treats that box as invalid); count_out = kept; scores_out[k] = its score as
 *      read, 0.0f beyond; index_out[k] = its candidate index, -1 beyond.
 * HOW (csrc/k_select.hip): the rank launch (grid: 256 candidates per workgroup x frame) prepares each candidate and finds its position
 * in the order of step 6 by COUNTING the members that precede it -- ranks are a permutation, so nothing is sorted and no atomic's order
 * matters -- and stores the members of rank < pre_nms_k into `scratch`; the suppress launch (one wave per frame) holds the working list
 * in LDS, walks it and writes every output.  `scratch` (device, 8-byte aligned, cvgs_boxes_select_scratch_bytes(max_candidates,
 * pre_nms_k) bytes -- 0 for arguments out of range) belongs to the call from its enqueue to the end of the suppress launch; its
 * contents before and after are unspecified.
 * Validation happens completely on the host before the first HIP call (a machine without a GPU can test it): null descriptors, null
 * boxes / scores / scratch / boxes_out / count_out, struct_size, flags, n outside 1..16, frame_width / frame_height < 1, a bad
 * box_format, max_candidates outside 1..65535, box_stride < 4, score_stride < 1, class_stride < 1 with classes, pre_nms_k outside
 * 1..1024, max_out outside 1..pre_nms_k, misaligned pointers (4 bytes; scratch: 8), iou_threshold outside [0, 1] or NaN, a NaN
 * score_threshold, sx or sy not finite or <= 0, ox or oy not finite, output or scratch buffers of one call that overlap ->
 * CVGS_ERR_INVALID; a frame beyond CVGS_MAX_DIM -> CVGS_ERR_UNSUPPORTED.
 *   cvgs_boxes_select_host  the same descriptor with HOST boxes / scores / classes / count; desc's scratch and output pointers are
 *                           ignored and the results go to boxes_out (float[max_out][4]), count_out, scores_out and index_out (the last
 *                           two optional).  Runs the shared text on the CPU and writes the bytes the kernels must write; makes no
 *                           HIP call.
 * No reference counterpart.                                                                                                          */
typedef enum cvgs_cand_format { CVGS_CAND_XYXY_F32 = 0, CVGS_CAND_CXCYWH_F32 = 1 } cvgs_cand_format;
#define CVGS_SELECT_MAX_FRAMES 16
#define CVGS_SELECT_MAX_PRE_NMS 1024
typedef struct cvgs_box_select_desc {
    uint32_t struct_size, flags;          /* sizeof(cvgs_box_select_desc); flags: must be 0 */
    int32_t frame_width, frame_height;    /* 1..CVGS_MAX_DIM: what the boxes are clamped into */
    int32_t box_format, max_candidates;   /* cvgs_cand_format; 1..65535 */
    const float* boxes;                   /* device: candidate i at boxes[i * box_stride + 0..3] */
    const float* scores;                  /* device: candidate i at scores[i * score_stride] */
    const int32_t* classes;               /* device: candidate i at classes[i * class_stride], or NULL (class-agnostic) */
    const int32_t* count;                 /* device, or NULL = max_candidates */
    int32_t box_stride, score_stride;     /* in floats: >= 4, >= 1 */
    int32_t class_stride, pre_nms_k;      /* in int32: >= 1 with classes; 1..CVGS_SELECT_MAX_PRE_NMS */
    int32_t max_out, reserved;            /* 1..pre_nms_k; 0 */
    float score_threshold, iou_threshold; /* not NaN; [0, 1] */
    float xform[4];                       /* (sx, sy, ox, oy): frame = detector * s + o */
    void* scratch;                        /* device, 8-byte aligned, cvgs_boxes_select_scratch_bytes(max_candidates, pre_nms_k) */
    float* boxes_out;                     /* device float[max_out][4] */
    int32_t* count_out;                   /* device int32 */
    float* scores_out;                    /* device float[max_out], or NULL */
    int32_t* index_out;                   /* device int32[max_out], or NULL */
} cvgs_box_select_desc;
size_t cvgs_boxes_select_scratch_bytes(int32_t max_candidates, int32_t pre_nms_k);
int cvgs_boxes_select(const cvgs_box_select_desc* descs, int32_t n, cvgs_stream_t stream); /* n = 1..CVGS_SELECT_MAX_FRAMES frames, one call */
int cvgs_boxes_select_host(const cvgs_box_select_desc* desc, void* boxes_out, int32_t* count_out, float* scores_out, int32_t* index_out);

/* ---- a detector's raw head -> the candidates cvgs_boxes_select reads ---------------------------------------------------------------------
 * What sits between a network's output tensor and cvgs_boxes_select.  Select reads four contiguous fp32 coordinates, one fp32 score and
 * one int32 class per candidate; exported heads offer none of that: YOLOv8 / v9 / v11 emit [4 + C, N] (channel-major), YOLOv5-style heads
 * [N, 5 + C] with an objectness value, both with C class scores per candidate and often in fp16 / bf16.  cvgs_head_decode enqueues TWO
 * small kernels on `stream` (csrc/k_head.hip: score, then compact) for up to 16 frames and nothing else: no allocation, no staging, no
 * copy, no synchronisation, so the call can be captured between the network and cvgs_boxes_select.  It reads the head in place through
 * two strides, reduces the class scores to (score, class), and hands select ONLY the candidates over the threshold, in candidate order,
 * with their number on the device: boxes_out / scores_out / classes_out / count_out are by construction a valid boxes (box_stride 4) /
 * scores (score_stride 1) / classes (class_stride 1) / count of a cvgs_box_select_desc with the same max_candidates.  The box format stays
 * the detector's (XYXY or CXCYWH): select converts and transforms as it does for any candidates.  Its cost: see README.md.
 *
 * Attribute a of candidate i is element head[i * cand_stride + a * attr_stride] (indexed in size_t, in elements of elem_type): a [N, A]
 * tensor is (A, 1), an [A, N] tensor is (1, N), padded rows or channels take a larger stride.  The four coordinates are the attributes
 * box_attr .. box_attr + 3, the class scores class_attr .. class_attr + num_classes - 1, the objectness value obj_attr (or -1: none).
 *
 * THE CONTRACT.  One text for the kernels and for cvgs_head_decode_host (csrc/cvgs_geometry.h: head_widen_f16 / head_widen_bf16,
 * head_best_step, head_best_wins, head_score, head_member), compiled with -ffp-contract=off, so the device writes the host entry's bytes.
 * Per frame, for every candidate i < max_candidates:
 *   1. WIDENING.  Every value read is widened to fp32, exactly: CVGS_HEAD_BF16 is the top 16 bits of an fp32; CVGS_HEAD_F16 widens exactly
 *      (subnormals included); CVGS_HEAD_F32 is read as it is.
 *   2. BEST CLASS.  best = -inf, cls = 0; for c = 0 .. num_classes - 1 in order, with v the class score of c: if (v > best) { best = v;
 *      cls = c; }.  A NaN never wins; among scores that compare equal the lowest class index wins (-0.0f equals 0.0f); best carries the
 *      winner's bits.  EQUIVALENT PARALLEL FORM (a wave reduction may use it): the maximum under "(v, c) beats (b, cb) iff (v > b) ||
 *      (v == b && c < cb)" over the non-NaN entries, with identity (-inf, 0).
 *   3. SCORE.  score = best; with obj_attr >= 0, score = obj * best: one fp32 multiplication, rounded once.
 *   4. MEMBERSHIP.  i is a MEMBER iff score >= score_threshold and none of its four widened coordinates is NaN.  A NaN score (NaN
 *      objectness, inf * 0) fails the first test.
 *   5. COMPACTION.  Members are compacted in candidate-index order.  The k-th member, counted from 0, is written as boxes_out[k] = its four
 *      widened coordinates as read, scores_out[k] = its score, classes_out[k] = its cls, index_out[k] = its candidate index; count_out =
 *      the number of members.
 *   6. EVERY element is written on every call: elements at or beyond count_out get (0, 0, 0, 0), 0.0f, 0 and -1.
 * CONSEQUENCES.  No NaN is ever stored.  There is no division and no transcendental function; apart from the multiplication of step 3
 * every step is a comparison or a move.  Because order is preserved, select's tie rule ("lower index first") means the same on the
 * compacted list as on the dense one: cvgs_boxes_select over the decoder's outputs, with the same score_threshold, returns exactly what
 * it returns over the dense per-candidate (score, class) arrays -- only its index_out differs, and it maps back to candidate indices
 * through the decoder's index_out (which is what cvgs_points_gather, below, follows to the landmarks of kept candidates, and what a
 * caller gathers their masks with).
 * OUT OF SCOPE.  Heads are expected to hold probabilities (exported graphs apply the sigmoid themselves): there is no sigmoid / exp, no
 * anchor or DFL decoding and no device `count` INPUT.
 * HOW (csrc/k_head.hip): both launches have the grid (256 candidates per workgroup, frame).  The score launch computes steps 1-4 for every
 * candidate and stores its score, class and member flag, and the tile's member count (ballot + popcount, the four wave totals through LDS),
 * in `scratch`.  It has two forms, chosen on the host by stride: attr_stride != 1 (and any stride pair): one lane per candidate walking the
 * classes, so that with cand_stride == 1 a wave's load of one channel is one contiguous span; attr_stride == 1: a group of 4 .. 64 lanes
 * per candidate reads consecutive attributes and reduces under the parallel form of step 2.  The compact launch has every workgroup sum
 * the counts of the tiles in front of it (at most 256), pack its own members behind them, read the coordinates of members only, and zero
 * the part of its own range that lies at or beyond the total.  No atomic, no workgroup waits for another, nothing depends on the order in
 * which workgroups run.  `scratch` (device, 8-byte aligned, cvgs_head_decode_scratch_bytes(max_candidates) bytes -- 0 for an argument out
 * of range) belongs to the call from its enqueue to the end of the compact launch; its contents before and after are unspecified.
 * Validation happens completely on the host before the first HIP call (a machine without a GPU can test it): null descriptors, null
 * head / scratch / boxes_out / scores_out / classes_out / count_out, struct_size, flags, reserved, n outside 1..16, a bad elem_type,
 * max_candidates outside 1..65535, cand_stride or attr_stride < 1, num_classes outside 1..4096, an attribute index outside 0..8191
 * (box_attr + 3, class_attr + num_classes - 1, obj_attr -- which may also be -1), misaligned pointers (head: its element size; outputs:
 * 4 bytes; scratch: 8), a NaN score_threshold (-inf is allowed), output or scratch buffers of one call that overlap -> CVGS_ERR_INVALID.
 *   cvgs_head_decode_host  the same descriptor with a HOST `head`; desc's scratch and output pointers are ignored and the results go to
 *                          boxes_out (float[N][4]), scores_out, classes_out, index_out (optional) and count_out.  Runs the shared text on
 *                          the CPU and writes the bytes the kernels must write; makes no HIP call.
 * No reference counterpart.                                                                                                          */
typedef enum cvgs_head_elem { CVGS_HEAD_F32 = 0, CVGS_HEAD_F16 = 1, CVGS_HEAD_BF16 = 2 } cvgs_head_elem;
#define CVGS_HEAD_MAX_FRAMES 16
#define CVGS_HEAD_MAX_CLASSES 4096
#define CVGS_HEAD_MAX_ATTR 8191
typedef struct cvgs_head_desc {
    uint32_t struct_size, flags;          /* sizeof(cvgs_head_desc); flags: must be 0 */
    const void* head;                     /* device: attribute a of candidate i at element i * cand_stride + a * attr_stride */
    int32_t elem_type, max_candidates;    /* cvgs_head_elem; N: 1..65535 */
    int32_t cand_stride, attr_stride;     /* in elements: >= 1 */
    int32_t box_attr, obj_attr;           /* the first of four coordinate attributes; the objectness attribute or -1 */
    int32_t class_attr, num_classes;      /* the first of num_classes class-score attributes; 1..CVGS_HEAD_MAX_CLASSES */
    float score_threshold;                /* not NaN; -inf keeps every candidate without a NaN coordinate or score */
    int32_t reserved;                     /* 0 */
    void* scratch;                        /* device, 8-byte aligned, cvgs_head_decode_scratch_bytes(max_candidates) */
    float* boxes_out;                     /* device float[N][4] */
    float* scores_out;                    /* device float[N] */
    int32_t* classes_out;                 /* device int32[N] */
    int32_t* index_out;                   /* device int32[N], or NULL */
    int32_t* count_out;                   /* device int32 */
} cvgs_head_desc;
size_t cvgs_head_decode_scratch_bytes(int32_t max_candidates);
int cvgs_head_decode(const cvgs_head_desc* descs, int32_t n, cvgs_stream_t stream); /* n = 1..CVGS_HEAD_MAX_FRAMES frames, one call */
int cvgs_head_decode_host(const cvgs_head_desc* desc, float* boxes_out, float* scores_out, int32_t* classes_out, int32_t* index_out, int32_t* count_out);

/* ---- the landmarks of kept detections -> the points cvgs_warp_tables_from_points reads ----------------------------------------------------
 * The link between the box path and the aligned-crop path.  Face and pose detectors emit the landmarks as further attributes of each
 * candidate of the same raw head -- YOLOv8-pose / YOLO-face: [4 + 1 + K * 3, N] (x, y, confidence per point); SCRFD / RetinaFace exports:
 * [N, 4 + 1 + 2 K] -- and after cvgs_head_decode and cvgs_boxes_select the survivors are known only as two device index lists: select's
 * index_out into the compacted list, decode's index_out from there into the head.  cvgs_points_gather enqueues ONE small kernel on
 * `stream` (csrc/k_gather.hip) for up to 16 frames and nothing else: no allocation, no staging, no copy, no synchronisation, so the call
 * can be captured between cvgs_boxes_select and cvgs_warp_tables_from_points.  It reads the head in place (fp32 / fp16 / bf16, the two
 * strides of cvgs_head_desc), follows the indices to the raw candidates, maps every landmark to frame pixels with select's xform rule and
 * writes points_out: by construction a valid `points` of a cvgs_warp_table_desc with max_items = max_out and the same n_points, whose
 * `count` is select's own count_out.  Its cost: see README.md.
 *
 * Attribute a of candidate c is element head[c * cand_stride + a * attr_stride] (in size_t, in elements of elem_type), as for
 * cvgs_head_decode.  Point p has x at attribute point_attr + p * point_step, y at the next one and (conf_offset >= 2) a confidence at
 * point_attr + p * point_step + conf_offset.
 *
 * THE CONTRACT.  One text for the kernel and for cvgs_points_gather_host (csrc/cvgs_geometry.h: gather_live, gather_source,
 * gather_elem_index, gather_map, gather_point), compiled with -ffp-contract=off, so the device writes the host entry's bytes.  Per frame,
 * for every row j < max_out:
 *   1. live = clamp(kept_count ? *kept_count : max_out, 0, max_out).
 *   2. Row j is VALID iff j < live, k = kept_index[j] lies in [0, max_candidates) and -- with cand_index -- c = cand_index[k] lies in
 *      [0, max_candidates); without cand_index c = k.  cvgs_head_decode writes -1 behind its count, so a stale k fails here.  Nothing is
 *      dereferenced with an index that failed its test, and indices are read only for j < live: the call is SAFE WHATEVER THE DEVICE
 *      BUFFERS HOLD, like the table builders.
 *   3. A valid row, point p: x and y are widened to fp32 exactly (as cvgs_head_decode's step 1), then x = x * sx; x = x + ox (two
 *      roundings, no fma) and the same for y with sy, oy -- select's step 4.  A result that is NaN is stored as the ONE bit pattern
 *      0x7fc00000, so host and device cannot differ in a payload; +-inf is stored as it comes.  conf_out[j][p] = the widened confidence
 *      attribute as read; source_out[j] = c.
 *   4. An invalid row: every coordinate is 0x7fc00000, every confidence 0.0f, source_out[j] = -1.  NaN and not 0: three coincident zero
 *      points are a legal input of the AFFINE3 fit, whereas a non-finite coordinate is what cvgs_warp_tables_from_points rejects under
 *      both fits -- even for a caller who forgets to pass the count.
 *   5. EVERY output element is written on every call.
 * The coordinates are NOT clamped: a landmark outside the frame is a legitimate input of a fit.
 * THE XFORM is the caller's, (sx, sy, ox, oy) as in cvgs_box_select_desc: frame = detector * s + o.  For a detector whose coordinates are
 * EDGE coordinates of its letterboxed input (pixel i spans [i, i + 1), as boxes are) it is select's own.  The warp kernels take integer
 * coordinates as PIXEL CENTRES (cv::warpAffine's convention), as do landmark heads trained on such coordinates: a detector that reports
 * pixel-centre coordinates in its input needs ox + 0.5 * sx - 0.5 (and oy + 0.5 * sy - 0.5) in place of ox (oy).
 * HOW (csrc/k_gather.hip): grid (ceil(max over frames of max_out * n_points / 256), frame), 256 work-items; work-item t of a frame owns
 * (j, p) = (t / n_points, t % n_points), so consecutive lanes store consecutive (x, y) pairs and a wave's store is one contiguous span;
 * the lane with p == 0 stores source_out[j].  The descriptors travel in the kernel arguments.  No LDS, no atomic.  The work is a few
 * thousand elements: the launch boundary is the cost.
 * Validation happens completely on the host before the first HIP call (a machine without a GPU can test it): null descriptors, null
 * head / kept_index / points_out, struct_size, flags, reserved, n outside 1..16, a bad elem_type, max_candidates or max_out outside
 * 1..65535, cand_stride or attr_stride < 1, point_step < 2, n_points outside 1..64, a conf_offset other than -1 or outside
 * [2, point_step), conf_out without conf_offset or conf_offset without conf_out, an addressed attribute outside 0..8191 (point_attr;
 * point_attr + (n_points - 1) * point_step + max(1, conf_offset)), misaligned pointers (head: its element size; everything else: 4
 * bytes), sx or sy not finite or <= 0, ox or oy not finite, output buffers of one call that overlap -> CVGS_ERR_INVALID.
 *   cvgs_points_gather_host  the same descriptor with HOST head / kept_index / kept_count / cand_index; desc's output pointers are ignored
 *                            and the results go to points_out (float[max_out][n_points][2]), conf_out (given exactly when conf_offset
 *                            is) and source_out (optional).  Runs the shared text on the CPU and writes the bytes the kernel must write;
 *                            makes no HIP call.
 * No reference counterpart.                                                                                                          */
#define CVGS_GATHER_MAX_FRAMES 16
#define CVGS_GATHER_MAX_POINTS 64
typedef struct cvgs_point_gather_desc {
    uint32_t struct_size, flags;          /* sizeof(cvgs_point_gather_desc); flags: must be 0 */
    const void* head;                     /* device: attribute a of candidate i at element i * cand_stride + a * attr_stride */
    int32_t elem_type, max_candidates;    /* cvgs_head_elem; 1..65535 */
    int32_t cand_stride, attr_stride;     /* in elements: >= 1 */
    int32_t point_attr, point_step;       /* x of point p = attribute point_attr + p * point_step, y = that + 1; point_step >= 2 */
    int32_t n_points, conf_offset;        /* 1..CVGS_GATHER_MAX_POINTS; the confidence of point p = attribute point_attr + p * point_step + conf_offset, or -1: none */
    int32_t max_out, reserved;            /* 1..65535; 0 */
    const int32_t* kept_index;            /* device int32[max_out]: select's index_out */
    const int32_t* kept_count;            /* device int32, or NULL = max_out: select's count_out */
    const int32_t* cand_index;            /* device int32[max_candidates], or NULL: decode's index_out (kept_index then indexes the compacted list) */
    float xform[4];                       /* (sx, sy, ox, oy): frame = detector * s + o */
    float* points_out;                    /* device float[max_out][n_points][2] */
    float* conf_out;                      /* device float[max_out][n_points], or NULL (required NULL when conf_offset == -1) */
    int32_t* source_out;                  /* device int32[max_out], or NULL: the raw candidate index of each row, -1 for an invalid row */
} cvgs_point_gather_desc;
int cvgs_points_gather(const cvgs_point_gather_desc* descs, int32_t n, cvgs_stream_t stream); /* n = 1..CVGS_GATHER_MAX_FRAMES frames, one call */
int cvgs_points_gather_host(const cvgs_point_gather_desc* desc, float* points_out, float* conf_out, int32_t* source_out);

#ifdef __cplusplus
}
#endif
#endif /* CVGS_HIP_EXT_H */
