/*
 * cu2rec_amd.h -- C ABI of the MI355X-native cu2rec hot path (libcu2rec_amd.so).
 *
 * Plain C: pointers, sizes, PODs.  No torch / HIP types in any signature (streams travel as
 * void*, device buffers as raw pointers).  Every entry point returns CU2REC_OK (0) or a
 * negative cu2rec_status; cu2rec_last_error() gives the message of the calling thread's last
 * failure.  The reference reports failures by throwing std::runtime_error from CHECK_CUDA
 * (util.h:27-34) or by printing to stderr and returning an empty result (util.cu:41-44); the
 * C++ wrappers in cu2rec_amd/csrc/cu2rec.hpp turn a non-zero status back into that exception.
 *
 * Each declaration names the reference interface it replaces
 * (paths relative to nickgreenquist/cu2rec matrix_factorization/).
 *
 * Device data layout ("padded rows"): dense factor matrices are row-major float32 with a row
 * stride `ld` that is a multiple of 4 floats (16 B) and >= n_factors; the padding floats must
 * be zero (they then stay zero under every kernel here).  ld == n_factors is the reference's
 * own layout (matrix.h:21-28) whenever n_factors % 4 == 0.  Recommended for Q, and what cu2rec_model uses: a stride of
 * a multiple of 32 floats, i.e. item rows that are whole 128-byte lines -- several XCDs read and write them, and rows
 * that share a line cost coherence misses and partial-line write-backs.  CSR is exactly the reference's:
 * int32 indptr[rows+1], int32 indices[nnz], float32 data[nnz] (matrix.h:11-19).
 */
#ifndef CU2REC_AMD_H
#define CU2REC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CU2REC_AMD_VERSION 100 /* 0.1.0 */

typedef enum cu2rec_status {
    CU2REC_OK = 0,
    CU2REC_EINVAL = -1,   /* bad argument (null pointer, bad shape, unsorted ratings, ...) */
    CU2REC_EIO = -2,      /* file cannot be opened / parsed */
    CU2REC_EHIP = -3,     /* a HIP runtime call failed (the reference's CHECK_CUDA throw) */
    CU2REC_ENODEVICE = -4,/* no usable GPU: the hot path never falls back to the CPU */
    CU2REC_ENOMEM = -5,
    CU2REC_EUNSUPPORTED = -6 /* e.g. n_factors above the compiled kernel range */
} cu2rec_status;

const char *cu2rec_last_error(void);
int cu2rec_version(void);
/* number of visible HIP devices, 0 if none (never fails) */
int cu2rec_device_count(void);
/* select the device used by subsequent calls of this thread (hipSetDevice) */
int cu2rec_set_device(int device);

/* ------------------------------------------------------------------------------------------
 * Config -- replaces config::Config (config.h:20-58) and its file format (config.cu:7-22).
 * The first nine fields are the file's nine whitespace separated fields, in file order.
 * The `__constant__` mirror (config.h:9-18, config.cu:24-48) has no equivalent: hyper-parameters
 * are passed to kernels by value (cu2rec_hyper below).
 * ---------------------------------------------------------------------------------------- */
typedef struct cu2rec_config {
    int cur_iterations;        /* config.h:23 */
    int total_iterations;      /* config.h:25  (default 5000) */
    int n_factors;             /* config.h:27  (default 50) */
    float learning_rate;       /* config.h:29  (default 0.01) */
    int seed;                  /* config.h:31  (default 42): sampler seed, training.cu:88 */
    float P_reg;               /* config.h:33  (default 0.02) */
    float Q_reg;               /* config.h:35 */
    float user_bias_reg;       /* config.h:37 */
    float item_bias_reg;       /* config.h:39 */
    int is_train;              /* config.h:41: 0 freezes Q and item_bias (honoured here; the
                                  reference never uploads it, config.cu:24-35) */
    int n_threads;             /* config.h:43 (default 32): kept for schema compatibility and
                                  printed; launch geometry is chosen by the library */
    int check_error;           /* config.h:45 (default 500) */
    float patience;            /* config.h:48 (default 2) */
    float learning_rate_decay; /* config.h:51 (default 0.2) */
} cu2rec_config;

int cu2rec_config_default(cu2rec_config *cfg);
int cu2rec_config_read(const char *path, cu2rec_config *cfg);        /* Config::read_config  config.cu:7-13 */
int cu2rec_config_write(const char *path, const cu2rec_config *cfg); /* Config::write_config config.cu:15-22 */
int cu2rec_config_print(const cu2rec_config *cfg);                   /* Config::print_config config.cu:50-64 (stdout) */

/* ------------------------------------------------------------------------------------------
 * Ratings file -> host CSR.  Replaces readCSV (util.cu:17-45) and the host half of
 * createSparseMatrix (util.cu:152-179).
 * ---------------------------------------------------------------------------------------- */
typedef struct cu2rec_ratings cu2rec_ratings; /* opaque, host memory */

/* "userId,itemId,rating" with one header line; ids 1-based, converted to 0-based.  rows/cols
 * = max id seen, global_bias = float(double sum / n).  A file that cannot be opened is
 * CU2REC_EIO (the reference prints "ERROR: The file isnt open." and returns nothing).
 * Files above ~1 MB whose records sit one per line are parsed on all host cores (CU2REC_READER_THREADS
 * overrides the count); anything else takes the sequential path, whose record grammar is the reference's
 * (`int char int char float` separated by arbitrary whitespace, first malformed record ends the file). */
int cu2rec_ratings_read_csv(const char *path, cu2rec_ratings **out);
/* Binary cache of a parsed file (header + three COO columns): loading it replaces the text parse. */
int cu2rec_ratings_save_binary(const cu2rec_ratings *r, const char *path);
int cu2rec_ratings_load_binary(const char *path, cu2rec_ratings **out);
int cu2rec_ratings_info(const cu2rec_ratings *r, int *n, int *rows, int *cols, float *global_bias);
/* raw COO views (length n), valid until cu2rec_ratings_free */
int cu2rec_ratings_view(const cu2rec_ratings *r, const int **user, const int **item, const float **rating);
void cu2rec_ratings_free(cu2rec_ratings *r);
/* Build the CSR into caller memory: indptr[rows+1], indices[n], data[n].  Users without
 * ratings get repeated pointers (tests/test_util.cu:146-189).  Ratings must be grouped by
 * ascending user (CU2REC_EINVAL otherwise -- the reference would not terminate); item order
 * inside a user is kept as in the file.  rows must be >= the largest user id. */
int cu2rec_csr_build(const cu2rec_ratings *r, int rows, int *indptr, int *indices, float *data);

/* initialize_normal_array (util.cu:124-144): std::mt19937(seed) +
 * std::normal_distribution<float>(mean, stddev / n_factors), sequential fill. */
int cu2rec_init_normal(float *out, size_t size, int n_factors, float mean, float stddev, int seed);

/* writeCSV / writeToFile (util.cu:86-103): "%f" comma joined rows;
 * file name <parent_dir>/<base>_f<factors>_<component>.csv */
int cu2rec_write_csv(const char *path, const float *data, int rows, int cols);
int cu2rec_write_component(const char *parent_dir, const char *base, const char *component, const float *data,
                           int rows, int cols, int factors);
/* read_array (util.cu:52-81): comma separated float rows; *out is malloc'ed -> cu2rec_free */
int cu2rec_read_array(const char *path, float **out, int *rows, int *cols);
void cu2rec_free(void *p);

/* ------------------------------------------------------------------------------------------
 * Sampler.  Replaces initCurand + curand_uniform (sgd.cu:11-16,36-37).  Counter based, no
 * state array, no init kernel: the draw of (user, iteration) is the first word of
 * rocRAND's Philox4x32-10 stream rocrand_init(seed, subsequence=user, offset=4*iteration),
 * mapped to (0,1] as rocrand_uniform does, then y_i = ceil(u * n) - 1 + low  (sgd.cu:37).
 * Host copy of the device function, for tests and for callers that need the schedule.
 * ---------------------------------------------------------------------------------------- */
uint32_t cu2rec_sampler_draw(uint64_t seed, uint64_t user, uint64_t iteration);
int cu2rec_sampler_index(uint64_t seed, uint64_t user, uint64_t iteration, int low, int high);

/* ------------------------------------------------------------------------------------------
 * Hot path on raw device pointers.  These are what a maintainer binds when the buffers
 * already live on the GPU (the reference's kernel-level interface, sgd.h:12-16, loss.h:18-24).
 * All pointers are device pointers on the current device unless marked host.  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous unless they
 * return host results.
 * Streams: what the library owns -- a cu2rec_schedule's workspace, the process-wide state of the resident launches -- it orders
 * itself: a call that uses it on another stream than its previous call starts behind that call, and the library's internal streams
 * start behind everything queued on `stream` ahead of the call.  Ordering the caller's own buffers across streams stays the
 * caller's duty.  One exception to "asynchronous": cu2rec_sgd_update_blocksolve waits on the host for `stream` on a schedule's
 * first block-solve call and whenever ldq differs from the schedule's previous call (it re-allocates a workspace sized by ldq).
 * ---------------------------------------------------------------------------------------- */
typedef struct cu2rec_hyper { /* the kernel-visible subset of config (config.h:9-18) */
    float learning_rate, P_reg, Q_reg, user_bias_reg, item_bias_reg;
} cu2rec_hyper;

typedef enum cu2rec_sgd_mode {
    /* One 16-lane group per user, all users of an iteration in flight at once; P, user_bias
     * updated in place by their owner, Q / item_bias rows updated in place with plain stores
     * (Hogwild: concurrent updates of one item overwrite each other, sgd.cu:18-21).  The
     * throughput path. */
    CU2REC_SGD_HOGWILD = 0,
    /* One group walks the users in ascending order: mf_sequential.cu:102-143 exactly
     * (in-place Gauss-Seidel).  Bit-identical to the CPU oracle in its TREE16 dot order.
     * For parity tests; orders of magnitude slower. */
    CU2REC_SGD_SERIAL = 1,
    /* The sequential result at GPU speed, deterministic, no races: the sample stream is value independent,
     * so each iteration is scheduled ahead of time as independent per-item chains whose updates run in
     * ascending user order with the item row held in registers (cu2rec_amd/csrc/ordered.hip).
     * Bit-identical to CU2REC_SGD_SERIAL and to the CPU oracle.  Needs a cu2rec_schedule workspace
     * (the object layer creates one per cu2rec_csr on first use; there the schedule lives in windows of up to 64 iterations
     * that outlive the call -- a call of any length, continuing the last one or not, runs out of the window that holds its
     * iterations, and the window behind it is scheduled beside them; with raw pointers no window outlives the call: the
     * arrays are the caller's). */
    CU2REC_SGD_ORDERED = 2,
    /* The reference GPU kernel's OWN semantics (sgd.cu:22-75 with the loop of training.cu:107-171), for callers that
     * want those trajectories rather than mf_sequential.cu's: every user reads the item side as it was at the start
     * of the iteration, the FIRST user to claim an item (sgd.cu:49-50) writes its new row / bias into a second buffer
     * pair, the pairs swap after every iteration (training.cu:164-165), an item nobody sampled falls back to its value
     * of two iterations ago.  "First" -- a race on a non-atomic flag in the reference -- is the lowest thread index
     * here (thread gid handles user (gid + 250 * iteration) % rows, training.cu:97-98,115), decided with a 64-bit
     * atomicMin, so the mode is deterministic and race free; the reference's surplus threads (grid = rows / n_threads
     * + 1 blocks, which update a few users twice) are not reproduced.  Object layer only (cu2rec_model_sgd,
     * cu2rec_train, bin/mf -m pingpong) or cu2rec_sgd_update_pingpong below. */
    CU2REC_SGD_PINGPONG = 3,
    /* mf_sequential.cu:102-143's semantics at Hogwild-class speed: the schedule of CU2REC_SGD_ORDERED, but the chain of
     * a popular item (thousands of dependent updates per iteration) is solved in blocks of 64 updates -- a block's errors
     * are the solution of a unit lower triangular 64 x 64 system built from the Gram matrix of its 64 user rows (fp32
     * matrix cores); its inverse, formed tile-wise ahead of the chain (two 32 x 32 triangular inversions + two matrix
     * products), turns 64 dependent row updates into three mat-vecs per block (cu2rec_amd/csrc/blocksolve.hip).  This is
     * the default of bin/mf and of bench.py, the mode certified against the north star's 1e-4 RMSE bar.  Equal to the
     * sequential result up to float rounding (sums are associated differently), NOT bit for bit: tests pin it at
     * |test RMSE - oracle| <= 1e-4 after 1,000 iterations of the ML-20M shape.  n_factors <= 252.  Needs a
     * cu2rec_schedule like CU2REC_SGD_ORDERED.  A call whose decay factors 1 - learning_rate * Q_reg or
     * 1 - learning_rate * item_bias_reg (in double) are at or below zero has no block form: it runs the ordered walk and
     * is the sequential result bit for bit. */
    CU2REC_SGD_BLOCKSOLVE = 4,
    /* Not an SGD mode: alternating least squares (cu2rec_model_als below), accepted by cu2rec_train only.  cu2rec_model_sgd,
     * the raw-pointer entry points and the sharded driver refuse it (CU2REC_EINVAL). */
    CU2REC_ALS = 5
} cu2rec_sgd_mode;

/* Replaces sgd_update (sgd.cu:22-75) + the per-iteration launch loop of train()
 * (training.cu:107-115): runs iterations [iter0, iter0 + n_iters), one update per user with
 * at least one rating per iteration.  update_items == 0 is is_train == false.
 * user_offset: global id of row 0 (0 unless the rows are one shard of a user-sharded set); it only
 * enters the sampler, so a shard draws exactly what the unsharded run draws for the same users. */
int cu2rec_sgd_update(const int *indptr, const int *indices, const float *data, int n_rows, int n_cols,
                      float *P, int ldp, float *Q, int ldq, float *user_bias, float *item_bias, float global_bias,
                      int n_factors, const cu2rec_hyper *hyper, uint64_t seed, uint64_t iter0, int n_iters,
                      int mode, int update_items, int user_offset, void *stream);

/* sgd_update (sgd.h:12-16) with its Q_target / item_bias_target / item_is_updated arguments, n_iters iterations with the
 * swap of training.cu:164-165 after each one: CU2REC_SGD_PINGPONG on raw device pointers.  Q_target / item_bias_target:
 * second buffers of the same shapes, initialised by the caller as copies of Q / item_bias (training.cu:37,69-70);
 * claim: n_cols 64-bit words of workspace (the role of item_is_updated; no per-iteration memset, reset by the call).
 * The buffers swap ROLES like the reference's pointers: *swapped = 1 means the current item side is now in
 * Q_target / item_bias_target (an odd number of swaps).  swap_last == 0 leaves out the last iteration's swap, so that
 * a loss evaluated right after the call sees what the reference's does (training.cu:121-137 run before the swap). */
int cu2rec_sgd_update_pingpong(const int *indptr, const int *indices, const float *data, int n_rows, int n_cols,
                               float *P, int ldp, float *Q, float *Q_target, int ldq, float *user_bias,
                               float *item_bias, float *item_bias_target, unsigned long long *claim,
                               float global_bias, int n_factors, const cu2rec_hyper *hyper, uint64_t seed,
                               uint64_t iter0, int n_iters, int update_items, int user_offset, int swap_last,
                               int *swapped, void *stream);

/* Optional sample array for the Hogwild path: [nnz] x {int32 item, float32 rating} = indices[k] and data[k] of the
 * CSR side by side (8 bytes per rating, device memory, 8-byte aligned), so that drawing a rating (sgd.cu:36-44) is
 * one 8-byte gather instead of two 4-byte gathers in different arrays.  The reference's CSR stays the input
 * format; this is a derived copy the caller owns: allocate cu2rec_sample_pairs_bytes(nnz), fill it once with
 * cu2rec_sample_pairs_build, pass it to cu2rec_sgd_update_ex (NULL = gather from indices / data; results are
 * identical either way).  Used by the resident launches (below); the owned-object layer (cu2rec_model_sgd,
 * cu2rec_train) keeps one per cu2rec_csr by itself. */
size_t cu2rec_sample_pairs_bytes(int nnz);
int cu2rec_sample_pairs_build(const int *indices, const float *data, int nnz, void *pairs, void *stream);
int cu2rec_sgd_update_ex(const int *indptr, const int *indices, const float *data, int n_rows, int n_cols,
                         float *P, int ldp, float *Q, int ldq, float *user_bias, float *item_bias, float global_bias,
                         int n_factors, const cu2rec_hyper *hyper, uint64_t seed, uint64_t iter0, int n_iters,
                         int mode, int update_items, int user_offset, const void *sample_pairs, void *stream);

/* Resident Hogwild launches (process-wide; replaces the launch loop of training.cu:107-113 with ONE persistent
 * launch per cu2rec_sgd_update call).  The iterations of a call keep the reference's cadence -- every user's update
 * of iteration i is visible to iteration i+1 -- but the boundary between them is a grid-wide barrier instead of a
 * kernel boundary, and every user's row stays in the register file for the whole call (no P traffic between
 * iterations).  Applies when all user rows of the CSR fit the register file + LDS (e.g. 204,000 users at f <= 128);
 * otherwise the call runs one streaming launch per iteration as before.
 * policy: 0 never, 1 auto (default: when it fits and a call covers >= 4 iterations), 2 whenever it fits;
 * CU2REC_RESIDENT=0|1|2 in the environment sets the initial value.  Returns the previous policy; other values query.
 * A resident launch assumes the GPU to itself (one workgroup per CU, all co-resident).  It is a cooperative launch: a
 * grid the runtime finds too large to be co-resident is refused up front and that call runs one streaming launch per
 * iteration instead (cu2rec_hogwild_resident_refusals counts them) -- nothing is lost.  What a launch-time check cannot
 * see (another process taking CUs while the grid runs) ends at the barrier's 3 s timeout: the next call into the library
 * returns CU2REC_EHIP (once: the model state is undefined after that, but the library stays usable, e.g. with policy 0). */
int cu2rec_hogwild_resident(int policy);
/* resident launches refused at launch time on the current device since the process started (those calls streamed) */
int cu2rec_hogwild_resident_refusals(void);
/* Waits for the current device and reports a resident launch that gave up at its barrier (CU2REC_EHIP, once), without
 * doing any other work: the same check every SGD / loss entry point makes on its way in. */
int cu2rec_check_faults(void);
/* 1 if a Hogwild cu2rec_sgd_update call of n_iters iterations on n_rows users would be one resident launch on the
 * current device under the current policy (then *blocks = workgroups, one per CU, and *users_per_group = rows each
 * 16-lane group keeps in registers; both may be NULL), 0 if it would stream, < 0 on error. */
int cu2rec_hogwild_resident_plan(int n_rows, int n_factors, int n_iters, int *blocks, int *users_per_group);

/* The arithmetic behind cu2rec_hogwild_resident_plan, without a device: 1 if the rows of n_rows users of n_factors floats
 * fit the registers + LDS of n_cus CUs (then *blocks = workgroups, *users_per_group = rows per 16-lane group, of which
 * *lds_rows live in LDS; all may be NULL), 0 if they do not.  Policy and call length are not considered. */
int cu2rec_hogwild_resident_geometry(int n_rows, int n_factors, int n_cus, int *blocks, int *users_per_group,
                                     int *lds_rows);
/* Partial residency (round 4; n_factors <= 256: every row width with a compiled partial form): a set too large for the chip still
 * runs as ONE launch per call -- of the users_per_group users of every group (cu2rec_hogwild_resident_geometry's figure INCLUDES the
 * streamed ones) the first users_per_group - s are resident as above, the other s streamed through the same pipeline, row in,
 * update, row out (the reference's loop is sgd.cu:22-75 either way).  Returns s for the geometry above: 0 = fully resident, > 0 = that
 * many streamed rows per group, -1 = no compiled form holds the set (one launch per iteration). */
int cu2rec_hogwild_resident_streamed_rows(int n_rows, int n_factors, int n_cus);

/* Workspace of CU2REC_SGD_ORDERED for one device CSR: item popularity ranks, key/value buffers of the
 * per-iteration schedule, sort scratch.  indptr / indices are device pointers (read once at creation). */
typedef struct cu2rec_schedule cu2rec_schedule;
int cu2rec_schedule_create(const int *indptr, const int *indices, int n_rows, int n_cols, int nnz,
                           cu2rec_schedule **out);
void cu2rec_schedule_destroy(cu2rec_schedule *s);
/* cu2rec_sgd_update in CU2REC_SGD_ORDERED mode on raw device pointers (same arguments + the workspace). */
int cu2rec_sgd_update_ordered(cu2rec_schedule *schedule, const int *indptr, const int *indices, const float *data,
                              int n_rows, int n_cols, float *P, int ldp, float *Q, int ldq, float *user_bias,
                              float *item_bias, float global_bias, int n_factors, const cu2rec_hyper *hyper,
                              uint64_t seed, uint64_t iter0, int n_iters, int update_items, int user_offset,
                              void *stream);

/* cu2rec_sgd_update in CU2REC_SGD_BLOCKSOLVE mode on raw device pointers (same arguments as the ordered form).
 * Launch topology: an iteration is phases 1-3 on `stream` and the other items' chains on a side stream of the schedule's.  Two forms,
 * same kernels, same bytes, same results (tests/test_gpu_blocksolve.py runs both): DEVICE -- fork and join by a gate kernel, a signal
 * kernel and one waiting workgroup, no event on the main stream; needs kernels of the two streams running SIDE BY SIDE -- and EVENTS
 * (3-6 us per iteration slower; works wherever HIP works).  The library picks per device, on the first block-solve call:
 *   1. CU2REC_BS_GATE=0 / 1 in the environment forces events / device;
 *   2. under a counter pass of rocprofv3 (--pmc; the tool exports ROCPROF_COUNTER_COLLECTION: kernels are serialised across streams):
 *      events -- so a --pmc pass is for counters, never for timing;
 *   3. otherwise a two-stream handshake probe on the streams the iterations will use (a wait kernel queued first on one, satisfied by a
 *      signal kernel on the other, 10 ms bound, both directions): streams sharing one hardware queue (GPU_MAX_HW_QUEUES=1), a tool that
 *      serialises dispatches, another tenant holding the compute units all end in events;
 *   4. a join that gives up mid-run (CU2REC_EHIP from the call or cu2rec_check_faults: the model state is undefined) switches the
 *      device to events for every later call of the process, and the error text says so.
 * cu2rec_blocksolve_topology reports what is in force.
 * Environment knobs the library reads (all optional, read once per process): CU2REC_RESIDENT (Hogwild launch form), CU2REC_BLOCKSOLVE_RATE,
 * CU2REC_BLOCKSOLVE_LOOKAHEAD, CU2REC_BS_GATE, CU2REC_BS_WAIT_S (block-solve mode), CU2REC_READER_THREADS, CU2REC_RATINGS_CACHE (ingest),
 * CU2REC_COMM_TIMEOUT_S, CU2REC_MERGE_ADAPTIVE_C, CU2REC_RCCL_WORLD1 (sharded driver; the last one a debugging aid: a real one-rank
 * communicator) -- ten in all; fault injection exists only in the test builds (make test-hooks). */
int cu2rec_sgd_update_blocksolve(cu2rec_schedule *schedule, const int *indptr, const int *indices, const float *data,
                                 int n_rows, int n_cols, float *P, int ldp, float *Q, int ldq, float *user_bias,
                                 float *item_bias, float global_bias, int n_factors, const cu2rec_hyper *hyper,
                                 uint64_t seed, uint64_t iter0, int n_iters, int update_items, int user_offset,
                                 void *stream);
/* Which items CU2REC_SGD_BLOCKSOLVE solves block-wise: those expected to receive at least `rate` updates per
 * iteration (sum over the item's raters of 1 / the rater's number of ratings); the other chains are walked update by
 * update.  Process-wide, read when a schedule is created; default 240 per 131,072 rating users, scaled with the set (no
 * less than 30: one GPU's shard of a strong-scaling run has shorter chains and the same launch overheads; the Netflix
 * shape's 480,189 users give 880); a value set here or by CU2REC_BLOCKSOLVE_RATE in the environment is taken as it is.
 * rate > 0 sets an explicit threshold, rate < 0 returns to the automatic one, rate == 0 only queries.  Returns what was in
 * force before the call: the explicit threshold, or -1 for automatic (so passing a returned value back restores it). */
float cu2rec_blocksolve_min_rate(float rate);
/* The longest chains in the look-ahead form (block-solve mode, n_factors <= 116; round 4; default: items expected to collect 24 blocks
 * and more per iteration -- the two or three longest chains of the ML-20M shape: -2.7 % per iteration).  Items EXPECTED to collect at
 * least `blocks` x 64 updates per iteration (the leading popularity ranks): phase 1 also builds, for every block of their chains
 * but the first, the 64 x 64 block of lr L that couples it to the block before it, and phase 2 runs the chain with
 *     e_i = M_i (pre_i - N_i e_(i-1))
 * -- two 64 x 64 matrix-vector products on ONE wavefront as the only dependent work per block, the item row following one block
 * behind on other wavefronts (no meeting points; DESIGN.md section 4, "The look-ahead form").  Same results as the plain form
 * up to float rounding.  Process-wide, read when a schedule is created (like cu2rec_blocksolve_min_rate); 0 = off;
 * CU2REC_BLOCKSOLVE_LOOKAHEAD in the environment sets the initial value.  Returns the previous value; blocks < 0 only queries. */
int cu2rec_blocksolve_lookahead_blocks(int blocks);
/* The fork / join form in force on the current device (see cu2rec_sgd_update_blocksolve): 2 device-side gate and join, 0 events,
 * -1 not decided yet (no block-solve call so far).  `why` (may be NULL): the reason, NUL-terminated, truncated to `cap` bytes. */
int cu2rec_blocksolve_topology(char *why, size_t cap);

/* Replaces calculate_loss_gpu + get_error_metrics_gpu (loss.cu:19-49,150-200) in ONE pass:
 * residual e = r - (gb + ub + ib + p.q) per rating, sum |e| and sum e^2 accumulated in
 * double, MAE = S1/n, RMSE = sqrt(S2/n) returned as float (loss.cu:185-190).
 * errors_out (device, nnz floats) may be NULL; when given it receives the residuals like the
 * reference's error_d array (loss.cu:31).  workspace: device memory of at least
 * cu2rec_loss_workspace_bytes() bytes.  Synchronises `stream` (host results).
 * ALWAYS size the workspace by calling cu2rec_loss_workspace_bytes(): it is NOT a constant of the ABI.  It grew by 16 bytes in
 * round 3 (the per-block partial sums are added on the device and the two results live at the workspace's tail: 2 x 4,096 + 2
 * doubles); a buffer sized by an older formula would be written past its end. */
size_t cu2rec_loss_workspace_bytes(void);
int cu2rec_loss(const int *indptr, const int *indices, const float *data, int n_rows, int nnz,
                const float *P, int ldp, const float *Q, int ldq, const float *user_bias, const float *item_bias,
                float global_bias, int n_factors, float *errors_out, void *workspace, double *sum_abs,
                double *sum_sq, float *mae, float *rmse, void *stream);

/* Replaces total_loss_kernel<B> + calculate_error_metric_gpu x2 (loss.cu:58-128,150-200) on an
 * explicit device array of residuals (tests/test_loss.cu:106-147). */
int cu2rec_error_metrics(const float *errors, int n, void *workspace, float *mae, float *rmse, void *stream);

/* ------------------------------------------------------------------------------------------
 * Owned device objects.  Replace CudaCSRMatrix / CudaDenseMatrix (matrix.h:11-28,
 * matrix.cu:12-46): constructor = allocate + H2D, destroy = free, download = to_host.
 * ---------------------------------------------------------------------------------------- */
typedef struct cu2rec_csr cu2rec_csr;     /* device CSR */
typedef struct cu2rec_model cu2rec_model; /* device P, Q, user_bias, item_bias + global_bias */

int cu2rec_csr_create(int rows, int cols, int nnz, const int *indptr, const int *indices, const float *data,
                      cu2rec_csr **out); /* host arrays in, CudaCSRMatrix ctor matrix.cu:28-40 */
int cu2rec_csr_info(const cu2rec_csr *m, int *rows, int *cols, int *nnz);
int cu2rec_csr_device_ptrs(const cu2rec_csr *m, const int **indptr, const int **indices, const float **data);
void cu2rec_csr_destroy(cu2rec_csr *m);
/* How many items CU2REC_SGD_BLOCKSOLVE solves block-wise on this rating matrix (creates its schedule on first use); 0 = the
 * mode is the ordered walk there.  < 0 on error. */
int cu2rec_csr_blocksolve_items(const cu2rec_csr *train);

/* Host arrays are dense (row stride n_factors), the reference's layout; any of P/Q/biases may
 * be NULL = initialise like the reference: initialize_normal_array(..., seed 42)
 * (training.cu:28,54,212-213). */
int cu2rec_model_create(int rows, int cols, int n_factors, const float *P, const float *Q, const float *user_bias,
                        const float *item_bias, float global_bias, cu2rec_model **out);
int cu2rec_model_info(const cu2rec_model *m, int *rows, int *cols, int *n_factors, int *ld, float *global_bias);
/* *ld above is the row stride of P (n_factors rounded up to 4 floats); this is the row stride of Q: n_factors rounded up
 * to 32 floats, so that every item row is a whole number of 128-byte cache lines (see "Device data layout"). */
int cu2rec_model_item_stride(const cu2rec_model *m);
/* The device arrays of the model (padded rows: P with stride ld, Q with cu2rec_model_item_stride).  Q / item_bias always name the CURRENT item side: after a
 * CU2REC_SGD_PINGPONG call they may be other buffers than before (the mode swaps two pairs), so ask again. */
int cu2rec_model_device_ptrs(const cu2rec_model *m, float **P, float **Q, float **user_bias, float **item_bias);
/* dense host arrays out (any may be NULL): CudaDenseMatrix::to_host + bias copies, training.cu:180-185 */
int cu2rec_model_download(const cu2rec_model *m, float *P, float *Q, float *user_bias, float *item_bias);
void cu2rec_model_destroy(cu2rec_model *m);

int cu2rec_model_sgd(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, uint64_t seed,
                     uint64_t iter0, int n_iters, int mode, int update_items);
int cu2rec_model_loss(const cu2rec_model *m, const cu2rec_csr *ratings, double *sum_abs, double *sum_sq,
                      float *mae, float *rmse);

/* ------------------------------------------------------------------------------------------
 * Scoring and ranking for MANY users at once -- replaces predict_ratings (predict.cu:17-30) and get_recommendations
 * (predict.cu:49-65), which the reference runs on the host for its one user.
 * scores[u * cols + i] = ((gb + ub[u]) + ib[i]) + p_u . q_i for every user of the model and every item: one dense
 * product on the matrix cores (f32 in, f32 accumulate).  The sum over the factors is associated differently from the
 * reference's sequential loop: equal up to float rounding.
 * ---------------------------------------------------------------------------------------- */
int cu2rec_model_scores(const cu2rec_model *m, float *scores_device /* rows * cols floats */, void *stream);
int cu2rec_model_scores_host(const cu2rec_model *m, float *scores_host /* rows * cols floats */);
/* For every user the k best items it has NOT rated, best predicted rating first.  rated: a CSR whose row u holds user
 * u's ratings (NULL: nothing is excluded; users past its last row are not masked).  items_out / scores_out: host arrays of
 * rows * k entries.  Rated items score -inf; a score whose radix code is at or below -inf's (-inf itself, and every NaN with its
 * sign bit set, which the descending sort puts after -inf) is never listed, so a user with fewer than k listable items gets
 * those, then -1 / NaN padding, never a hole.  Items with equal scores come out in ascending item index (the sort is stable). */
int cu2rec_model_recommend(const cu2rec_model *m, const cu2rec_csr *rated, int k, int *items_out, float *scores_out);
/* The k best non-excluded items of each listed user, without the dense score matrix: scores on the matrix cores and
 * selection on chip, workspace bounded by a batch of users (not by rows x cols).  Scores and order are recommend's, bit for
 * bit: the same float score; descending in rocPRIM's float radix order (+0.0 and -0.0 tie, +NaN above +inf), ties by
 * ascending item; a score of -inf is never listed; -1 / NaN padding when fewer than k candidates remain.  exclude: row u holds
 * user u's excluded items (unsorted, repeats allowed; NULL: nothing; rows past its last row exclude nothing).  users: host
 * list of n_users model rows (duplicates allowed), or NULL for every row of the model (n_users ignored).  items_out /
 * scores_out: host, n_users x k.  1 <= k <= 256; a larger k is CU2REC_EUNSUPPORTED (cu2rec_model_recommend ranks any k). */
int cu2rec_model_topk(const cu2rec_model *m, const cu2rec_csr *exclude, const int *users, int n_users, int k,
                      int *items_out, float *scores_out);
/* Nearest neighbours of factor rows among the rows of the same matrix, on cu2rec_model_topk's tile and selection.
 * side: CU2REC_SIDE_USERS (rows of P) or CU2REC_SIDE_ITEMS (rows of Q).  ids: host list of n_ids rows of that side
 * (duplicates allowed), or NULL for every row (n_ids ignored).  The candidates of query row a are every row b != a of the
 * side: the query row itself is never listed, however often it is asked for.
 *   CU2REC_SIM_DOT:    score = x_a . x_b, no biases; the same MFMA contraction as cu2rec_model_scores.
 *   CU2REC_SIM_COSINE: score = u_a . u_b on the same contraction, u_r = x_r / |x_r| computed in double and rounded to float
 *                      by a pre-pass over the side's rows (recomputed on every call: nothing is cached on the model), so
 *                      any row of finite floats with a nonzero norm, subnormal or near FLT_MAX, is scored within float
 *                      rounding of its float64 cosine.  The pre-pass holds the unit rows in rows x ld floats of device memory
 *                      for the call (55 MB for the users of ML-20M at f = 100).  A row of norm 0 has cosine 0 (+0.0 or -0.0) with every
 *                      row, as query and as candidate.  A row holding an inf or a NaN scores +NaN (0x7FC00000) with every
 *                      row, as query and as candidate: listed first by the radix order, whatever the NaN's origin.
 * exclude: row a holds the rows excluded for query row a (topk's rules: unsorted, repeats allowed, NULL: nothing, rows past its
 * last row exclude nothing; rows and ids must be below the side's row count).  Order, ties, -inf and padding are topk's, with
 * row ids in place of items.  ids_out / scores_out: host, n x k.  1 <= k <= 256, else CU2REC_EUNSUPPORTED; a bad side, metric
 * or id is CU2REC_EINVAL, checked before the device is touched. */
enum { CU2REC_SIDE_USERS = 0, CU2REC_SIDE_ITEMS = 1 };
enum { CU2REC_SIM_DOT = 0, CU2REC_SIM_COSINE = 1 };
int cu2rec_model_similar(const cu2rec_model *m, int side, int metric, const cu2rec_csr *exclude, const int *ids, int n_ids,
                         int k, int *ids_out, float *scores_out);
/* The k users with the best predicted rating for each listed item: score ((gb + ub[u]) + ib[i]) + p_u . q_i, bit for bit the
 * float cu2rec_model_scores writes at [u, i] (P stays the A operand of the contraction).  exclude: row i holds item i's excluded
 * users, e.g. the training set transposed (HostCSR.transpose() in Python); topk's rules otherwise.  items: host list of n_items
 * item ids (duplicates allowed), or NULL for every item.  Order, ties, -inf, padding and the range of k are topk's, with user
 * ids in place of items.  users_out / scores_out: host, n x k. */
int cu2rec_model_top_users(const cu2rec_model *m, const cu2rec_csr *exclude, const int *items, int n_items, int k,
                           int *users_out, float *scores_out);
/* Ranking quality of the model's top-k lists (cu2rec_model_topk over every row, excluding `exclude`) against a test set.
 * For each model row u:
 *   R_u = distinct items of test row u with rating >= threshold (threshold -INFINITY: every rating; NaN: CU2REC_EINVAL).
 *         Items >= the model's cols count in |R_u| but are never hit; R_u is not reduced by `exclude`.
 *   Users with |R_u| = 0 are skipped and counted.  Test rows past the model's rows: CU2REC_EINVAL.
 *   L_u = the top-k list without padding; hits = |L_u n R_u|.
 *   precision = hits / k (k even when L_u is shorter); recall = hits / |R_u|; hit = [hits > 0];
 *   ndcg = DCG / IDCG, DCG = sum over j with L_u[j] in R_u of 1 / log2(j + 2), IDCG = sum over j < min(k, |R_u|) of the same;
 *   ap = (1 / min(k, |R_u|)) * sum over j with L_u[j] in R_u of (hits in L_u[0..j]) / (j + 1).
 * Each reported value is the mean over evaluated users, summed in double on the device (NaN when no user is evaluated).
 * per_user (host, may be NULL): rows x 5 doubles {precision, recall, ndcg, ap, hit}, NaN for skipped users. */
typedef struct cu2rec_rank_metrics {
    int k, users_evaluated, users_skipped;
    double precision, recall, ndcg, map, hit_rate;
} cu2rec_rank_metrics;
int cu2rec_model_rank_metrics(const cu2rec_model *m, const cu2rec_csr *exclude, const cu2rec_csr *test, int k,
                              float threshold, cu2rec_rank_metrics *out, double *per_user);

/* ------------------------------------------------------------------------------------------
 * Alternating least squares.  SGD (every mode above) takes stochastic steps on
 *   L = 1/2 sum_(u,i) in train (r_ui - gb - ub_u - ib_i - p_u . q_i)^2
 *     + 1/2 sum_u n_u (P_reg |p_u|^2 + user_bias_reg ub_u^2) + 1/2 sum_i m_i (Q_reg |q_i|^2 + item_bias_reg ib_i^2)
 * (n_u: ratings of user u in the CSR, m_i: entries naming item i; repeated pairs count separately; gb fixed).  One ALS half-step
 * minimises L exactly over one side with the other frozen.  Users: for each user u with n_u >= 1, x = [p_u; ub_u], z_i = [q_i; 1],
 * t_ui = r_ui - gb - ib_i, solve (sum_i z_i z_i^T + n_u diag(P_reg, ..., P_reg, user_bias_reg)) x = sum_i t_ui z_i.  Items: the
 * same with y = [q_i; ib_i], w_u = [p_u; 1], t = r - gb - ub_u, Q_reg, item_bias_reg and m_i.
 * The Gram is formed on the matrix cores in f32 (v_mfma_f32_32x32x2_f32), the system solved by Cholesky in LDS (f32).  A row's
 * result depends only on its own ratings and the partner side -- never on the batch, the other rows or the run: bit-identical
 * across runs, and a user fitted from a one-user CSR equals the same user fitted with all the others.  The result overwrites the
 * row's factors (padding floats written as zero) and its bias.  Left unchanged: rows with no ratings, model rows past the CSR's
 * rows / items, the other side, and every row whose factorisation meets a pivot that is not a finite positive float or whose
 * solution is not finite (e.g. a row that gathers an inf or a NaN) -- these are counted in *unsolved (may be NULL).
 * side: CU2REC_SIDE_USERS (solve P, user_bias given Q, item_bias) or CU2REC_SIDE_ITEMS (the reverse).  hyper->learning_rate is
 * ignored.  CU2REC_EINVAL, checked before the device or the model is touched: a null m / train / hyper, a bad side, a factor
 * regulariser of the side (P_reg for users, Q_reg for items) that is not finite and > 0, a bias regulariser of the side that is
 * not finite and >= 0 (negative, NaN, inf), ratings past the model's shape.  n_factors > CU2REC_ALS_MAX_FACTORS: CU2REC_EUNSUPPORTED.
 * A pending ping-pong swap is finished first.  The first item half-step on a cu2rec_csr builds its item-major view on the device
 * (nnz x 8 bytes, kept with the cu2rec_csr).
 * Length thresholds: a row's ratings are staged CU2REC_ALS_STEP at a time; rows of at most CU2REC_ALS_CHUNK ratings are solved by
 * one workgroup; longer rows are cut into ceil(n / CU2REC_ALS_CHUNK) chunks (at most CU2REC_ALS_MAX_CHUNKS: longer rows get longer
 * chunks, in whole steps) whose partial Grams are summed in chunk order.  Workspace: the long rows go in batches of whole rows whose
 * partial Grams (P x 4 KiB each, P = T (T + 1) / 2 tile pairs, T = ceil((n_factors + 2) / 32)) fit CU2REC_ALS_WORKSPACE_BYTES
 * (64 MiB: 1,638 chunks at n_factors 100, 455 at 252) -- whatever the row count; allocated on the first long row, kept with the
 * cu2rec_csr.
 * ---------------------------------------------------------------------------------------- */
enum { CU2REC_ALS_MAX_FACTORS = 252, CU2REC_ALS_STEP = 32, CU2REC_ALS_CHUNK = 1024, CU2REC_ALS_MAX_CHUNKS = 64,
       CU2REC_ALS_WORKSPACE_BYTES = 64 << 20 };
int cu2rec_model_als(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, int side, int *unsolved);
/* The same half-step by conjugate gradients: an approximate solver, warm-started from the row's current values, that never forms
 * the row's Gram.  In the notation above (x = [factors; bias], z_i = [partner factors; 1], t_i = (r_i - gb) - partner bias, n the
 * row's ratings, D = n_factors + 1) the system is applied as an operator,
 *   A v = sum_i z_i (z_i . v) + n diag(reg, ..., reg, reg_bias) v,   b = sum_i t_i z_i,
 * and a row is treated by its length:
 *   0 ratings: the row keeps its values and is not counted -- as above.
 *   more than CU2REC_ALS_CHUNK ratings: solved exactly by the kernels of cu2rec_model_als, bit for bit what that call writes.  Long
 *     rows are solved exactly whatever cg_steps is.
 *   1 .. CU2REC_ALS_CHUNK ratings: x0 = [the row's n_factors factors; its bias] (the padding floats are never read as data; if any
 *     of the D values is not finite, x0 = 0); r = b - A x0, p = r, rho = r . r; then cg_steps times: if rho == 0 stop and keep x;
 *     d = p . A p; if d == 0 stop and keep x; a = rho / d; x += a p; r -= a A p; rho' = r . r; p = r + (rho' / rho) p; rho = rho'
 *     -- the iteration of cu2rec_model_als_implicit_cg below.  Factors and bias are both written, the padding floats as 0.
 * A row is left with the bits it had and counted in *unsolved when a rho or a d is not finite, a d is negative or the final x is
 * not finite (e.g. a NaN rating, a partner row that overflows).
 * Determinism as above: every sum's order is a function of the row's own length and n_factors, there are no float atomics,
 * results are bit-identical run to run, and a row solved from a one-row CSR equals that row solved among all the others.  One
 * wavefront per row; there is no global Gram, so nothing is staged and no workspace is used by these rows.
 * cg_steps must lie in [1, CU2REC_ALS_CG_MAX_STEPS] (256, below), else CU2REC_EINVAL, checked -- like everything cu2rec_model_als
 * checks, with the same codes -- before the device or the model is touched. */
int cu2rec_model_als_cg(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, int side, int cg_steps, int *unsolved);

/* ------------------------------------------------------------------------------------------
 * Implicit feedback: confidence-weighted alternating least squares (Hu, Koren, Volinsky: Collaborative Filtering for Implicit
 * Feedback Datasets, ICDM 2008).  Every user x item pair of the CSR's shape counts: U = train rows, I = train cols, each stored
 * entry (u, i, r) is an observation of weight w = alpha * r (repeated pairs count separately), s_ui = p_u . q_i; there are no
 * biases and no global bias:
 *   L = 1/2 sum_(u < U, i < I) s_ui^2 + 1/2 sum_entries (w (1 - s_ui)^2 + 1 - 2 s_ui)
 *     + 1/2 P_reg sum_(u < U) |p_u|^2 + 1/2 Q_reg sum_(i < I) |q_i|^2
 * -- for pairs stored once, sum c (p - s)^2 with c = 1 + w, p = 1 on stored pairs and c = 1, p = 0 elsewhere.  The regulariser is
 * plain reg here, NOT n_u reg / m_i reg as in the explicit objective above.
 * A user half-step solves, for EVERY user u < U, with Y = Q[0:I]:
 *   (Y^T Y + sum_entries w q_i q_i^T + P_reg I_f) p_u = sum_entries (1 + w) q_i;
 * a user without entries has right-hand side 0: its row is written as zeros, not factorised and not counted.  The item half-step
 * is the mirror image on the item-major view with X = P[0:U] and Q_reg.  After a half-step the solved side's biases of the rows
 * inside the CSR are 0 and its padding floats are 0; model rows past the CSR's rows / cols and the whole other side keep their bits.
 * Y^T Y is formed once per half-step: the partner rows in tiles of CU2REC_ALS_CHUNK, one workgroup per tile on the explicit
 * half-step's matrix-core accumulation, the tiles' partial Grams added in tile order (in batches through the same workspace) --
 * a function of the partner rows alone.  A row's own sum starts from it and adds its entries exactly as the explicit half-step
 * does (same stage, chunk cut and chunk-order summation; the entries are staged as the two operands [w q | 1 + w] and [q | 0], so
 * w = 0 is an ordinary entry), then the order-f system is solved by the same Cholesky.  A row's result depends only on its own
 * entries and the partner rows [0, I) or [0, U): bit-identical across runs, and a user solved from a one-user CSR of the same cols
 * equals that user solved among all the others.  A row is left unchanged and counted in *unsolved (may be NULL) when a pivot is
 * not a finite positive float (possible only with negative or non-finite data) or its solution is not finite.
 * CU2REC_EINVAL, checked before the device or the model is touched: a null m / train / hyper, a bad side, a factor regulariser of
 * the side that is not finite and > 0, alpha not finite or < 0, a CSR whose rows or cols exceed the model's.  The bias
 * regularisers and the learning rate are ignored.  n_factors > CU2REC_ALS_MAX_FACTORS: CU2REC_EUNSUPPORTED.  Single GPU.
 * ---------------------------------------------------------------------------------------- */
int cu2rec_model_als_implicit(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, int side,
                              int *unsolved);
/* The same half-step by conjugate gradients (Takacs, Pilaszy, Tikk: Applications of the conjugate gradient method for implicit
 * feedback collaborative filtering, RecSys 2011): an approximate solver, warm-started from the row's current factors, that never
 * forms the row's Gram.  With A v = G0 v + sum_entries w (q . v) q + reg v applied as an operator (G0 = X^T X over the partner
 * rows inside the CSR, formed as above) and b = sum_entries (1 + w) q, a row is treated by its length:
 *   0 entries: written as zeros, not counted -- as above.
 *   more than CU2REC_ALS_CHUNK entries: solved exactly by the kernels of cu2rec_model_als_implicit, bit for bit what that call
 *     writes.  Long rows are solved exactly whatever cg_steps is.
 *   1 .. CU2REC_ALS_CHUNK entries: x0 = the row's current n_factors factors (the padding floats are never read as data; if any
 *     of them is not finite, x0 = 0); r = b - A x0, p = r, rho = r . r; then cg_steps times: if rho == 0 stop and keep x;
 *     d = p . A p; if d == 0 stop and keep x; a = rho / d; x += a p; r -= a A p; rho' = r . r; p = r + (rho' / rho) p; rho = rho'.
 *     x is written with padding floats 0 and bias +0.0.
 * A row is left with the bits it had and counted in *unsolved when a rho or a d is not finite, a d is negative or the final x is
 * not finite.  CG does NOT promise to detect an indefinite system: negative weights are outside the model, and a row that holds
 * some may come back solved, wrong and uncounted (the Cholesky call above counts it).
 * Determinism as above: every sum's order is a function of the row's own length and n_factors, there are no float atomics,
 * results are bit-identical run to run, and a row solved from a one-row CSR of the same cols equals that row solved among all the
 * others.  One wavefront per row; G0 is unpacked once per call into a dense matrix of n_factors^2 floats kept with the cu2rec_csr.
 * cg_steps must lie in [1, CU2REC_ALS_CG_MAX_STEPS], else CU2REC_EINVAL, checked -- like everything cu2rec_model_als_implicit
 * checks, with the same codes -- before the device or the model is touched. */
enum { CU2REC_ALS_CG_MAX_STEPS = 256 };
int cu2rec_model_als_implicit_cg(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, int side,
                                 int cg_steps, int *unsolved);
/* *L = the objective above at the model's current values: the all-pairs term as 1/2 <P^T P, Q^T Q> from two global Grams (f32, as
 * the half-step forms them), the entries term and the two norms from one pass over the entries and the rows, summed in double
 * like the loss pass.  Regularisers >= 0 are accepted here.  Reads the model only. */
int cu2rec_model_implicit_objective(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, double *L);

/* ------------------------------------------------------------------------------------------
 * Implicit feedback: logistic matrix factorization (Johnson: Logistic Matrix Factorization for Implicit Feedback Data, 2014), in
 * its full-batch form.  U = train rows, I = train cols; every stored entry (u, i, r) has weight w = alpha * r (repeated pairs count
 * separately); the score is the one the ranking calls use, s_ui = global_bias + user_bias[u] + item_bias[i] + p_u . q_i, and
 * sigma(s_ui) is the probability that u interacts with i.  The log-posterior to be MAXIMISED is
 *   L = sum_entries w s_ui - sum_(u < U, i < I) softplus(s_ui) - sum_entries w softplus(s_ui)
 *     - 1/2 P_reg sum_(u < U) |p_u|^2 - 1/2 Q_reg sum_(i < I) |q_i|^2 - 1/2 user_bias_reg sum ub^2 - 1/2 item_bias_reg sum ib^2
 * (bias regularisers of 0: the paper's model).  global_bias is read, never trained.
 * A user half-step (the item half-step is its mirror image on the item-major view the ALS calls cache on the cu2rec_csr) forms,
 * for EVERY u < U -- a user without entries is an ordinary row, the all-pairs term still moves it --
 *   g_u  = sum_(entries of u) w (1 - sigma(s_ui)) q_i - sum_(i < I) sigma(s_ui) q_i - P_reg p_u
 *   gb_u = sum_(entries of u) w (1 - sigma(s_ui))     - sum_(i < I) sigma(s_ui)     - user_bias_reg ub_u
 * and then takes an AdaGrad step, element-wise in float32 without contraction, lr = hyper->learning_rate (no decay):
 *   a' = a + g g;   x' = x + (lr g) / sqrtf(a') where a' > 0, else x' = x.
 * The accumulators a, one float per factor and per bias, live with the cu2rec_model: allocated zeroed by the first logistic call,
 * untouched by every other call.  A row keeps its values AND its accumulators bit for bit, and is counted in *n_unchanged (may be
 * NULL), when any of its n_factors + 1 gradient values, new values or new accumulators is not finite.  Model rows past the CSR's
 * rows / cols and the whole other side keep their bits.
 * The all-pairs sum never forms the U x I matrix: 32 own rows per workgroup against the partner side 128 rows at a time, scored in
 * float32 on the matrix cores as cu2rec_model_top_users scores, sigma(s) pushed through a second matrix-core product against the
 * partner tile.  Every sum's order is a function of the partner index or the entry's position alone, there are no float atomics:
 * results are bit-identical run to run, a row's gradient from a one-row CSR of the same cols equals its gradient among all the
 * others, and the item half-step equals the user half-step of the transposed problem.
 * CU2REC_EINVAL, all checked before the device or the model is touched: a null m / train / hyper, a bad side, any of the four
 * regularisers not finite or < 0, alpha not finite or < 0, learning_rate not finite or <= 0, a CSR whose rows or cols exceed the
 * model's.  n_factors > CU2REC_ALS_MAX_FACTORS: CU2REC_EUNSUPPORTED.  Single GPU.
 * ---------------------------------------------------------------------------------------- */
int cu2rec_model_lmf(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, int side, int *n_unchanged);
/* The gradient cu2rec_model_lmf would step along, to the host: grad_out [n x n_factors] and bias_grad_out [n] (either may be
 * NULL), n = the CSR's rows (CU2REC_SIDE_USERS) or cols (CU2REC_SIDE_ITEMS).  The model and the accumulators are untouched. */
int cu2rec_model_lmf_gradient(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, int side,
                              float *grad_out, float *bias_grad_out);
/* *L = the log-posterior above at the model's current values: the all-pairs term from float32 matrix-core scores, softplus and
 * every sum in double (per lane, per workgroup, the workgroups in order); the entries' term and the norms from scores in double.
 * The same checks as cu2rec_model_lmf (no side), and L not NULL.  Reads the model only. */
int cu2rec_model_lmf_objective(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, float alpha, double *L);
/* The AdaGrad accumulators to the host, dense like cu2rec_model_download (any pointer may be NULL); zeros before the first
 * logistic call.  cu2rec_model_lmf_reset zeroes them. */
int cu2rec_model_lmf_state(cu2rec_model *m, float *aP, float *aQ, float *a_ub, float *a_ib);
int cu2rec_model_lmf_reset(cu2rec_model *m);

/* ------------------------------------------------------------------------------------------
 * Implicit feedback: Bayesian Personalized Ranking (Rendle, Freudenthaler, Gantner, Schmidt-Thieme: BPR: Bayesian Personalized
 * Ranking from Implicit Feedback, 2009) in a deterministic, full-batch form.  U = train rows, I = train cols; entry e = (u, i) is
 * the k-th stored entry of row u; stored values are not read; repeated pairs count separately.
 * Negatives.  For sweep t and entry (u, k), up to 8 attempts a = 0 .. 7 draw
 *   j = cu2rec_sampler_index(seed, u, ((uint64_t)(t * 8 + a) << 32) | k, 0, I)
 * and the first j that row u does not store is the entry's negative j_e; if all eight are stored items the entry has no triple in
 * this sweep (j_e = -1) and contributes nothing anywhere.  The draw depends on seed, u, k, t, I and the row's own set of items only.
 * Rows may be unsorted and hold repeats: the membership test is exact (a binary search of a row-sorted copy of the indices, cached
 * on the cu2rec_csr by the first call that needs it, as the item-major view is).  Both half-steps of a sweep use the same
 * negatives.  With x_e = (item_bias[i] - item_bias[j_e]) + p_u . (q_i - q_j) -- the user bias and the global bias cancel -- the
 * quantity to be MAXIMISED is
 *   L = sum_triples ln sigma(x_e) - 1/2 P_reg sum_(u < U) |p_u|^2 - 1/2 Q_reg sum_(i < I) |q_i|^2 - 1/2 item_bias_reg sum_(i < I) ib_i^2
 * (plain regularisers, as in cu2rec_model_als_implicit, not n * reg; user_bias_reg is checked and otherwise unused).
 * CU2REC_SIDE_USERS: for every u < U,  g_u = sum_(triples of u) sigma(-x_e) (q_i - q_j) - P_reg p_u;  the user bias' gradient is a
 * zero, and the step below leaves user_bias and its accumulator bit for bit as they were.
 * CU2REC_SIDE_ITEMS: for every i < I, with c_e = sigma(-x_e) at the current values,
 *   g_i  = sum_(e: item(e) = i) c_e p_u - sum_(e: j_e = i) c_e p_u - Q_reg q_i
 *   gb_i = sum_(e: item(e) = i) c_e     - sum_(e: j_e = i) c_e     - item_bias_reg ib_i
 * the positives first, in ascending position of the item-major view, then the negatives in ascending e (each dealt to four partial
 * sums by position, added in order); an item that is never a positive and never a negative gets -reg x.
 * Either side then takes cu2rec_model_lmf's AdaGrad step with its unchanged-row rule (any non-finite gradient value, new value or
 * new accumulator of a row -- a user's bias counts as its row's -- leaves the row's bits and is counted in *n_unchanged, may be
 * NULL) ON THE SAME ACCUMULATORS: the model has one set, which cu2rec_model_lmf_state / cu2rec_model_lmf_reset expose and both
 * trainers move; reset them between the two.  Model rows past the CSR and the frozen side keep their bits.
 * No float atomics, every sum's order is a function of positions alone: bit-identical run to run, and a user's gradient and
 * negatives in a CSR where every other row is empty equal those among the others.
 * CU2REC_EINVAL, all checked before the device or the model is touched: a null m / train / hyper, a bad side, any of the four
 * regularisers not finite or < 0, learning_rate not finite or <= 0, a CSR whose rows or cols exceed the model's, sweep outside
 * [0, 2^29).  n_factors > CU2REC_ALS_MAX_FACTORS: CU2REC_EUNSUPPORTED.  A CSR with cols == 0 or nnz == 0 is a valid problem
 * without triples.  Single GPU.
 * ---------------------------------------------------------------------------------------- */
int cu2rec_model_bpr(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, uint64_t seed, int sweep, int side,
                     int *n_unchanged);
/* The gradient cu2rec_model_bpr would step along, to the host, shaped as cu2rec_model_lmf_gradient's (either may be NULL).  The
 * model and the accumulators are untouched. */
int cu2rec_model_bpr_gradient(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, uint64_t seed, int sweep, int side,
                              float *grad_out, float *bias_grad_out);
/* *L = the objective above at the model's current values over sweep `sweep`'s triples: ln sigma(x_e) = -softplus(-x_e) from scores
 * in double, every sum in double with the workgroups' partial sums added in order.  *n_triples = the number of triples and
 * *n_ordered = the number with x_e > 0 (either may be NULL): n_ordered / n_triples is the sampled AUC.  The same checks (no side),
 * and L not NULL.  Reads the model only. */
int cu2rec_model_bpr_objective(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, uint64_t seed, int sweep, double *L,
                               long long *n_triples, long long *n_ordered);
/* neg_out[e] (host, nnz ints) = j_e of sweep `sweep`, or -1.  CU2REC_EINVAL: a null argument, sweep outside [0, 2^29). */
int cu2rec_csr_bpr_negatives(const cu2rec_csr *train, uint64_t seed, int sweep, int *neg_out);

/* ------------------------------------------------------------------------------------------
 * Implicit feedback: softmax matrix factorization -- matrix factorization under the multinomial likelihood of Mult-DAE / Mult-VAE
 * (Liang, Krishnan, Hoffman, Jebara: Variational Autoencoders for Collaborative Filtering, WWW 2018, sections 2-3), full batch.
 * U = train rows, I = train cols; a stored entry (u, i, r) has weight w = r (repeated pairs count separately; there is no alpha:
 * scaling w only rescales the likelihood against the regularisers); W_u = the sum of w over the entries of u.  The score is the
 * one the ranking calls and cu2rec_model_lmf use, s_ui = ((global_bias + user_bias[u]) + item_bias[i]) + p_u . q_i.  For user u
 * the items form ONE distribution and the user's interactions are draws from it:
 *   lse_u = log sum_(i < I) exp(s_ui)       (every item of train's shape, stored or not)
 *   pi_ui = exp(s_ui - lse_u)
 * global_bias and user_bias[u] cancel in pi, so neither is ever trained: user biases keep their bits.  To be MAXIMISED:
 *   L = sum_entries w (s_ui - lse_u) - 1/2 P_reg sum_(u < U) |p_u|^2 - 1/2 Q_reg sum_(i < I) |q_i|^2 - 1/2 item_bias_reg sum_(i < I) ib_i^2
 * (plain regularisers, as in cu2rec_model_lmf, not n * reg; user_bias_reg is not read).
 * CU2REC_SIDE_USERS, for every u < U:  g_u = sum_(entries of u) w q_i - W_u sum_(i < I) pi_ui q_i - P_reg p_u;  the user bias'
 * gradient is a zero; a user without entries only shrinks.
 * CU2REC_SIDE_ITEMS, for every i < I (on the item-major view the ALS calls cache on the cu2rec_csr):
 *   g_i  = sum_(u has i) w p_u - sum_(u < U) W_u pi_ui p_u - Q_reg q_i
 *   gb_i = sum_(u has i) w     - sum_(u < U) W_u pi_ui     - item_bias_reg ib_i
 * Either side then takes cu2rec_model_lmf's AdaGrad step at hyper->learning_rate, with its unchanged-row rule and its count
 * (*n_unchanged, may be NULL), ON THE SAME ACCUMULATORS: the model has one set, which cu2rec_model_lmf_state /
 * cu2rec_model_lmf_reset expose and the logistic, the BPR and the softmax calls all move; reset them between trainers.  The user
 * side adds a zero to the user bias and its accumulator.  Model rows past the CSR and the frozen side keep their bits.
 * Nothing of size U x I is formed.  Every call first takes W_u (the row's values added in entry order) and lse_u: 32 users per
 * workgroup against the items 128 at a time, scored in float32 on the matrix cores as cu2rec_model_lmf scores, with an online
 * max and sum per user (per lane over its 16 scores, the two halves of the wavefront, the wavefront's steps, the four wavefronts
 * in order; expf and logf, not the fast intrinsics).  The half-step then scores the pairs again -- the same bits, so
 * exp(s_ui - lse_u) cannot overflow -- and pushes the coefficient (pi_ui, or W_u pi_ui on the item side) through a second
 * matrix-core product against [partner rows | 1], as cu2rec_model_lmf pushes sigma.  Every sum's order is a function of the partner
 * index or the entry's position alone, there are no float atomics: results are bit-identical run to run, and a user's lse and
 * gradient from a one-row CSR of the same cols equal what it gets among all the others.
 * Non-finite values behave as they fall out of the arithmetic.  A user whose lse_u is not finite (a NaN or an infinity among its
 * factors, its bias or the item side) has a non-finite gradient: it is left unchanged and counted.  In an item half-step that
 * user's coefficients W_u pi_ui are NaN for every item -- also where W_u = 0, since 0 x NaN is NaN -- so every item is left
 * unchanged and counted.
 * CU2REC_EINVAL, all checked before the device or the model is touched: a null m / train / hyper, a bad side, P_reg, Q_reg or
 * item_bias_reg not finite or < 0, learning_rate not finite or <= 0, a CSR whose rows or cols exceed the model's.
 * n_factors > CU2REC_ALS_MAX_FACTORS: CU2REC_EUNSUPPORTED.  A CSR with cols == 0 or nnz == 0 is a valid problem.  Single GPU.
 * ---------------------------------------------------------------------------------------- */
int cu2rec_model_softmax(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, int side, int *n_unchanged);
/* The gradient cu2rec_model_softmax would step along, to the host, shaped as cu2rec_model_lmf_gradient's (either may be NULL); the
 * users' bias_grad_out is all zeros.  The model and the accumulators are untouched. */
int cu2rec_model_softmax_gradient(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, int side, float *grad_out,
                                  float *bias_grad_out);
/* *L = the objective above at the model's current values: lse_u in float32 as the half-steps form it, the entries' scores, the
 * term w (s_ui - lse_u) and every sum in double, the workgroups' partial sums added in order.  The same checks (no side), and L
 * not NULL.  Reads the model only. */
int cu2rec_model_softmax_objective(cu2rec_model *m, const cu2rec_csr *train, const cu2rec_hyper *hyper, double *L);
/* lse_out (host, U floats) = lse_u of every user inside the CSR, as the half-steps form it; -inf where cols == 0.
 * cu2rec_model_softmax_mass: mass_out (host, U floats) = sum_(i < I) pi_ui as the user half-step's matrix-core product forms it
 * (its column of ones), 1 within rounding: a check of the two passes against each other.  CU2REC_EINVAL: a null argument, a CSR
 * past the model's shape; CU2REC_EUNSUPPORTED as above.  Read the model only. */
int cu2rec_model_softmax_lse(cu2rec_model *m, const cu2rec_csr *train, float *lse_out);
int cu2rec_model_softmax_mass(cu2rec_model *m, const cu2rec_csr *train, float *mass_out);

/* ------------------------------------------------------------------------------------------
 * train() -- replaces both overloads of train (training.h:12-15, training.cu:21-217):
 * total_iterations iterations; loss on train and test when i == 0, (i+1) % check_error == 0
 * or last (training.cu:118) printed as "TRAIN: Iteration %d GPU MAE: %f RMSE: %f" / "TEST: ..."
 * (training.cu:135,137) when `verbose`; patience / learning-rate decay on the test RMSE
 * (training.cu:101-103,146-155, "New Learning Rate" line); "Time taken for %d of iterations
 * is %lf" (training.cu:177).  cfg->learning_rate and cfg->cur_iterations are updated as the
 * reference does (training.cu:152,170).  losses (host, total_iterations floats, may be NULL):
 * losses[i] = test RMSE at the checked iterations (training.cu:158), NaN elsewhere.
 * The model is updated in place; download it afterwards.
 * mode CU2REC_ALS: one iteration is one sweep -- cu2rec_model_als on the users, then on the items when cfg->is_train -- with the
 * same loss cadence, lines and losses; there is no learning rate, so no patience / decay: cfg->learning_rate stays as it is and no
 * "New Learning Rate" line is printed; stats->updates counts the rows solved.  n_factors > 252: CU2REC_EUNSUPPORTED.
 * ---------------------------------------------------------------------------------------- */
typedef struct cu2rec_train_stats {
    double seconds_total;  /* wall time of the loop, loss checks included (training.cu:106,172-177) */
    double seconds_sgd;    /* GPU time of the SGD launches only (HIP events) */
    double updates;        /* users-with-ratings x iterations */
    int n_checks;
    float last_train_mae, last_train_rmse, last_test_mae, last_test_rmse;
} cu2rec_train_stats;

int cu2rec_train(const cu2rec_csr *train, const cu2rec_csr *test, cu2rec_config *cfg, cu2rec_model *model,
                 int mode, int verbose, float *losses, cu2rec_train_stats *stats);
/* cu2rec_train's CU2REC_ALS loop, lines, cadence, losses and stats with sweeps of cu2rec_model_als_cg at cg_steps steps.  The same
 * argument checks with the same codes as cu2rec_train, and cg_steps outside [1, CU2REC_ALS_CG_MAX_STEPS]: CU2REC_EINVAL, all before
 * the device or the model is touched. */
int cu2rec_train_als_cg(const cu2rec_csr *train, const cu2rec_csr *test, cu2rec_config *cfg, cu2rec_model *model, int cg_steps,
                        int verbose, float *losses, cu2rec_train_stats *stats);
/* Implicit-feedback training: total_iterations sweeps of cu2rec_model_als_implicit -- the users, then the items when cfg->is_train
 * -- with the objective evaluated at the loss cadence above, printed as "TRAIN: Iteration %d GPU implicit objective: %f" when
 * `verbose`, and stored in objectives[i] (host, total_iterations doubles, may be NULL; NaN elsewhere).  There is no test set and no
 * learning rate: no decay, cfg->learning_rate stays as it is; cfg->cur_iterations advances.  stats->updates = rows solved (rows
 * without entries, written as zeros, are not counted); the stats' MAE / RMSE fields are 0. */
int cu2rec_train_implicit(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, float alpha, int verbose,
                          double *objectives, cu2rec_train_stats *stats);
/* cu2rec_train_implicit's loop, lines, cadence and stats with sweeps of cu2rec_model_als_implicit_cg at cg_steps steps
 * (cg_steps outside [1, CU2REC_ALS_CG_MAX_STEPS]: CU2REC_EINVAL before anything is touched). */
int cu2rec_train_implicit_cg(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, float alpha, int cg_steps,
                             int verbose, double *objectives, cu2rec_train_stats *stats);
/* Logistic matrix factorization training: the accumulators are reset, then total_iterations sweeps of cu2rec_model_lmf -- the users,
 * then the items when cfg->is_train -- at learning rate cfg->learning_rate (AdaGrad's own; no decay) with the log-posterior
 * evaluated at cu2rec_train_implicit's cadence, printed as "TRAIN: Iteration %d GPU logistic objective: %f" when `verbose`, and
 * stored in objectives[i] (may be NULL; NaN elsewhere).  stats->updates = rows stepped (rows left unchanged are not counted).
 * cu2rec_model_lmf's checks with its codes, before the device or the model is touched. */
int cu2rec_train_lmf(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, float alpha, int verbose, double *objectives,
                     cu2rec_train_stats *stats);
/* BPR training: the accumulators (the logistic trainer's) are reset, then total_iterations sweeps of cu2rec_model_bpr -- the users,
 * then the items when cfg->is_train -- with seed cfg->seed; sweep t is iteration t of cfg's count (cfg->cur_iterations + the
 * iterations done), so the last one must be below 2^29.  The objective over the triples of the sweep just done is evaluated at
 * cu2rec_train_implicit's cadence, printed as "TRAIN: Iteration %d GPU BPR objective: %f" when `verbose`, and stored in
 * objectives[i] (may be NULL; NaN elsewhere).  No decay.  stats->updates = rows stepped.  cu2rec_model_bpr's checks with its codes,
 * before the device or the model is touched. */
int cu2rec_train_bpr(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, int verbose, double *objectives,
                     cu2rec_train_stats *stats);
/* Softmax matrix factorization training: the accumulators (the logistic trainer's) are reset, then total_iterations sweeps of
 * cu2rec_model_softmax -- the users, then the items when cfg->is_train -- at learning rate cfg->learning_rate (no decay), with the
 * objective L evaluated at cu2rec_train_implicit's cadence, printed as "TRAIN: Iteration %d GPU softmax objective: %f" when
 * `verbose`, and stored in objectives[i] (may be NULL; NaN elsewhere).  stats->updates = rows stepped.  cu2rec_model_softmax's
 * checks with its codes, before the device or the model is touched. */
int cu2rec_train_softmax(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, int verbose, double *objectives,
                         cu2rec_train_stats *stats);

/* ------------------------------------------------------------------------------------------
 * Sharding by user (multi-GPU; the reference is single device).  Host-side planner:
 * user_begin[nranks+1] with contiguous ranges of (almost) equal user count; work per SGD
 * iteration is one update per user.
 * ---------------------------------------------------------------------------------------- */
int cu2rec_shard_plan(int rows, int nranks, int *user_begin);
/* Slice a host CSR to users [u0,u1): indptr_out[u1-u0+1] rebased to 0; returns the slice's
 * nnz in *nnz_out and the offset of its first rating in *offset_out (indices/data slices are
 * then plain sub-arrays). */
int cu2rec_csr_slice(const int *indptr, int rows, int u0, int u1, int *indptr_out, int *offset_out, int *nnz_out);
/* Expected number of SGD updates per iteration that the rows of a host CSR make on each item:
 * rate[y] = sum over users u that rated y of 1 / degree(u)   (each user samples uniformly among its ratings). */
int cu2rec_item_update_rates(const int *indptr, const int *indices, int n_rows, int n_cols, double *rate);

/* ------------------------------------------------------------------------------------------
 * User-sharded training on several GPUs, ONE PROCESS PER GPU (the reference is single device; the interface extended
 * is train(), training.h:12-15).  Each rank owns a contiguous user range -- its CSR slice (cu2rec_csr_slice), a model
 * whose P / user_bias cover the local users and whose Q / item_bias are a replica of the whole item side -- and every
 * sync_every iterations the replicas are reconciled by ONE sum all-reduce of the item deltas in their wire format,
 * n_cols * (n_factors + 1) floats without row padding: Q = Q_base + scale * sum_k w_k (Q_k - Q_base).  Sampler draws
 * are keyed by the global user id (user_offset), so a shard draws what the unsharded run draws.
 *
 * The communicator is RCCL over xGMI (resolved at run time with dlopen: a copy already in the process -- PyTorch's -- is
 * reused): created here from an ncclUniqueId the caller distributes (cu2rec_comm_unique_id on rank 0, 128 bytes), or an
 * ncclComm_t the caller already owns, handed in as void*.  For tests there is a callback form: the caller's own
 * in-place sum all-reduce on a device buffer (count elements of float, or double when is_double), ordered on `stream`
 * or synchronising it; return 0 on success.  Every rank must make the same sequence of job calls.
 * ---------------------------------------------------------------------------------------- */
typedef struct cu2rec_comm cu2rec_comm;
typedef int (*cu2rec_allreduce_fn)(void *ctx, void *device_buf, size_t count, int is_double, void *stream);
int cu2rec_comm_unique_id(void *id_out /* 128 bytes */);
int cu2rec_comm_create(const void *unique_id, int rank, int nranks, cu2rec_comm **out); /* ncclCommInitRank on the current device */
int cu2rec_comm_from_nccl(void *nccl_comm, int rank, int nranks, cu2rec_comm **out);    /* not owned */
int cu2rec_comm_from_callback(cu2rec_allreduce_fn fn, void *ctx, int rank, int nranks, cu2rec_comm **out);
void cu2rec_comm_destroy(cu2rec_comm *comm);
/* What the communicator really is, for a bench line / a preflight to PROVE the collective's world: rank / nranks as given at
 * creation; rccl_nranks / rccl_rank / rccl_device from ncclCommCount / ncclCommUserRank / ncclCommCuDevice of the attached
 * ncclComm_t (all 0 / -1 / -1 when no RCCL communicator is attached: one rank, or the callback form); rccl_version from
 * ncclGetVersion (0 if RCCL was never loaded).  Any pointer may be NULL. */
typedef struct cu2rec_comm_info_t {
    int rank, nranks;
    int rccl_nranks, rccl_rank, rccl_device;
    int rccl_version;
    int is_callback; /* 1: the caller's all-reduce (tests), no RCCL on the data path */
} cu2rec_comm_info_t;
int cu2rec_comm_info(const cu2rec_comm *comm, cu2rec_comm_info_t *out);

typedef enum cu2rec_merge {
    CU2REC_MERGE_MEAN = 0,     /* scale 1 / nranks */
    CU2REC_MERGE_WEIGHTED = 1, /* per item: w_k[y] = rank k's share of the item's expected updates per iteration */
    CU2REC_MERGE_SUM = 2,      /* scale 1: diverges when many ranks update the same items many times per period */
    CU2REC_MERGE_ADAPTIVE = 3  /* the sum, scaled per item by phi(r_total) / sum_k phi(r_k), phi(r) = 1 - exp(-c r), r = expected
                                * updates of the item per iteration, c = 6 * min(1, sync_every / epoch) (what saturates a row is its
                                * updates per PERIOD; CU2REC_MERGE_ADAPTIVE_C overrides c): the sum for rarely updated items, the mean
                                * for items every rank updates all the time.  ML-20M shape, 8 shards, 1,000 iterations: test RMSE 3e-4
                                * from the unsharded sequential result (mean / weighted: 1e-3) */
} cu2rec_merge;
typedef struct cu2rec_shard_options {
    int sync_every; /* iterations between exchanges; 0 = one epoch = round(nnz / users) of the whole population */
    int merge;      /* cu2rec_merge */
} cu2rec_shard_options;

typedef struct cu2rec_shard_job cu2rec_shard_job;
/* model and train must outlive the job; options may be NULL (epoch cadence, CU2REC_MERGE_ADAPTIVE: the default of bin/mf
 * and bench.py). Collective: all ranks call it. */
int cu2rec_shard_job_create(cu2rec_comm *comm, cu2rec_model *model, const cu2rec_csr *train, int user_offset,
                            const cu2rec_shard_options *options, cu2rec_shard_job **out);
void cu2rec_shard_job_destroy(cu2rec_shard_job *job);
/* n_iters iterations on the local shard, exchanging every sync_every iterations (the cadence runs across calls) */
int cu2rec_shard_job_run(cu2rec_shard_job *job, const cu2rec_hyper *hyper, uint64_t seed, uint64_t iter0, int n_iters,
                         int mode, int update_items);
/* an exchange out of cadence (if anything happened since the last one): every replica equal afterwards */
int cu2rec_shard_job_exchange(cu2rec_shard_job *job);
/* MAE / RMSE over all ranks' slices of `ratings` (all-reduce of sum |e|, sum e^2, n) */
int cu2rec_shard_job_loss(cu2rec_shard_job *job, const cu2rec_csr *ratings, double *sum_abs, double *sum_sq,
                          double *n_total, float *mae, float *rmse);
int cu2rec_shard_job_info(const cu2rec_shard_job *job, int *sync_every, int *exchanges, double *users_total,
                          double *nnz_total, size_t *wire_bytes);
/* Device time of the exchanges so far: every exchange (items_wire_pack -> all-reduce -> items_wire_apply) is bracketed by a pair
 * of events on its stream; `timed` of them have completed and been read (an exchange whose events were still in flight when
 * their slot was needed again is not counted), `seconds` is their sum on THIS rank -- it includes the wait for the slowest
 * peer.  Call after the stream has been synchronised to have every exchange counted.  Pointers may be NULL. */
int cu2rec_shard_job_exchange_stats(cu2rec_shard_job *job, int *timed, double *seconds, double *max_seconds);
/* cu2rec_train over all ranks: same schedule, same stdout lines (rank 0 prints), patience / learning-rate decay on the
 * GLOBAL test RMSE; `test` is the rank's slice of the test set; stats->updates counts the whole population. */
int cu2rec_train_sharded(cu2rec_shard_job *job, const cu2rec_csr *test, cu2rec_config *cfg, int mode, int verbose,
                         float *losses, cu2rec_train_stats *stats);

/* ------------------------------------------------------------------------------------------
 * Item-based nearest-neighbour recommendation (ItemKNN): no factors, no learning rate, no seed.  `train` is the user x item CSR
 * with I columns, n_u the number of entries user u stores.  Every stored entry gets a weight w_ui:
 *   CU2REC_KNN_COUNT   w = r
 *   CU2REC_KNN_COSINE  w = r / sqrt(sum_v r_vi^2)
 *   CU2REC_KNN_TFIDF   w = t / sqrt(sum_v t_vi^2), t_ui = sqrt(r_ui) idf_u, idf_u = ln(I) - ln(1 + n_u)
 *   CU2REC_KNN_BM25    w = r (k1 + 1) / (k1 len_i + r) idf_u, len_i = (1 - b) + b c_i / mean(c), c_i = sum_v r_vi, the mean over
 *                      all I columns (a zero denominator gives w = 0)
 * evaluated in double (the per-user and per-column sums in a fixed order, k1 and b as the floats given) and rounded to float once;
 * a column whose norm is 0 gets weights 0.  The similarity of two items is S_ij = sum_u w_ui w_uj over the users that store both;
 * item i keeps its N best neighbours among the TOUCHED candidates j != i (at least one user stores both i and j), whatever their
 * value.  A recommendation for a history row h (raw stored values r) scores score_j = sum_{i in h} r_i S_N[i, j] over the
 * truncated lists; candidates are the touched j (some history item lists j) outside the `exclude` row.
 *
 * Every score is the fold acc = fmaf(alpha, v, acc) from +0.0f in a fixed order -- the users of column i in ascending order for
 * S_ij, the history row's items in ascending id order for score_j -- with no float atomics: results are bit-identical run to
 * run, and a query alone gives what it gives among others.  Order, ties (ascending id) and the -1 / NaN padding of every list
 * are cu2rec_model_topk's; unlike there, a touched candidate is listed even when its value is -inf or NaN.
 *
 * Rows of every CSR may be unsorted (the library works on its own row-sorted copy, made on first use and kept with the
 * cu2rec_csr); a train or history row that stores the same column twice is CU2REC_EINVAL.  Null arguments, a weighting outside
 * the four, a non-finite or negative k1, b outside [0, 1], neighbours or k outside [1, 256], an id out of range, a history,
 * exclude or test CSR whose column count differs from the model's: CU2REC_EINVAL, checked before the device is touched where the
 * arguments alone show it.
 *
 * The product runs one wavefront per (query, slice of cu2rec_knn_slice_items() consecutive candidate ids), in batches of queries
 * whose workspace ((slices + 1) * k * 8 bytes per query) fits CU2REC_KNN_WORKSPACE_BYTES. */
enum { CU2REC_KNN_COUNT = 0, CU2REC_KNN_COSINE = 1, CU2REC_KNN_TFIDF = 2, CU2REC_KNN_BM25 = 3 };
enum { CU2REC_KNN_MAX_NEIGHBOURS = 256, CU2REC_KNN_WORKSPACE_BYTES = 64 << 20 };
typedef struct cu2rec_knn cu2rec_knn;
/* builds the model: weights, the N best neighbours of every item, and their id-sorted copy for cu2rec_knn_recommend */
int cu2rec_knn_create(const cu2rec_csr *train, int weighting, float k1, float b, int neighbours, cu2rec_knn **out);
void cu2rec_knn_destroy(cu2rec_knn *knn);
int cu2rec_knn_info(const cu2rec_knn *knn, int *items, int *neighbours, int *weighting); /* pointers may be NULL */
/* candidate ids per wavefront slice (a constant of the build; needs no device) */
int cu2rec_knn_slice_items(void);
/* w_ui of every stored entry, in the CSR's own entry order -> out_nnz (host, nnz floats) */
int cu2rec_csr_knn_weights(const cu2rec_csr *csr, int weighting, float k1, float b, float *out_nnz);
/* the k <= neighbours best neighbours of each listed item (ids: host, duplicates allowed; NULL: every item) -> host, n x k */
int cu2rec_knn_neighbors(const cu2rec_knn *knn, const int *ids, int n, int k, int *out_ids, float *out_sims);
/* the k best candidates of each listed history row (users: host row ids of `history`, duplicates allowed; NULL: every row; row u
 * of `exclude` -- may be NULL, rows past its last exclude nothing -- is not listed for row u) -> host, n x k */
int cu2rec_knn_recommend(const cu2rec_knn *knn, const cu2rec_csr *history, const cu2rec_csr *exclude, const int *users, int n,
                         int k, int *out_items, float *out_scores);
/* cu2rec_model_rank_metrics' definitions over cu2rec_knn_recommend's lists of every history row (the rows the means are taken
 * over; test rows past them: CU2REC_EINVAL).  per_user: host, history rows x 5, may be NULL. */
int cu2rec_knn_rank_metrics(const cu2rec_knn *knn, const cu2rec_csr *history, const cu2rec_csr *exclude, const cu2rec_csr *test,
                            int k, float threshold, cu2rec_rank_metrics *out, double *per_user);

/* ------------------------------------------------------------------------------------------
 * EASE (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", WWW 2019): a dense item x item weight matrix in closed form.
 * One hyper-parameter (l2), no factors, no seed, no iterations.  `train` is the user x item CSR with I columns, values r as stored
 * (the caller binarises if it wants to).
 *   G    the Gram matrix: off the diagonal G_ij is ItemKNN's CU2REC_KNN_COUNT similarity S_ij, the fold acc = fmaf(r_ui, r_uj, acc)
 *        from +0.0f over the users of column i in ascending order; on the diagonal G_ii = fl(sum_u r_ui^2 + l2), the sum in the same
 *        order and l2 added once, as the float given, to the finished float sum
 *   P    = G^-1 in float32 through the Cholesky factor G = L L^T: a blocked factorisation in place on the lower triangle (blocks of
 *        cu2rec_ease_block_items() items), the blocked triangular inverse of L, then L^-T L^-1
 *   B    B_ij = -P_ij / P_jj (an IEEE division) for i != j, B_ii = 0: the columns are scaled, B is not symmetric
 * The score of history row u for item j is sum_i r_ui B_ij over the row's stored entries in ascending item id (an entry that repeats
 * a column counts each time), the fold acc = fmaf(r, B_ij, acc) from +0.0f.  EVERY item that row u of `exclude` does not name is a
 * candidate -- also one whose score is 0 and one nobody stores, unlike ItemKNN's touched candidates -- so a list has
 * min(k, I - excluded) entries, best first, ties by ascending id, then cu2rec_model_topk's -1 / NaN padding.  The neighbours of item i
 * are that list for the one-entry history {i: 1.0} with i excluded: the k largest B_ij of row i.  An item nobody stores has
 * P_ii = 1 / l2 and a zero row and column of B.
 *
 * No float atomics; every sum is a fixed-order fmaf / matrix-core chain: a model built twice is bit-identical, results are
 * bit-identical run to run, and a query alone gives what it gives among others.
 *
 * Limits: one GPU; I <= CU2REC_EASE_MAX_ITEMS (more: CU2REC_EUNSUPPORTED, before anything is allocated); k in [1, CU2REC_EASE_MAX_K];
 * the inverse is float32.  The model holds one (I rounded up to whole blocks)^2 float matrix, in which every stage runs in place
 * beside O(I x block) of workspace; a matrix that does not fit is CU2REC_ENOMEM.  A pivot of the factorisation that is not a finite
 * number above the rounding noise of its own diagonal entry, 2^-22 G_jj (l2 too small for the data in float -- two identical columns
 * with l2 below an ulp of their sum of squares --, a NaN value) fails the whole build with CU2REC_EUNSUPPORTED, cu2rec_last_error()
 * naming the pivot's item, and *out stays NULL; nothing on the device traps.  cols == 0 or nnz == 0 is a valid model with nothing
 * (or only zero scores) to list.
 *
 * A train row that stores the same column twice, an l2 that is not finite or <= 0, k outside its range, an id out of range, null
 * arguments, a history, exclude or test CSR whose column count differs from the model's: CU2REC_EINVAL, checked before the device is
 * touched where the arguments alone show it.  Rows of every CSR may be unsorted.
 *
 * Lists come from one wavefront per (query, slice of cu2rec_knn_slice_items() consecutive ids), in batches of queries whose workspace
 * ((slices + 1) * k * 8 bytes per query) fits CU2REC_EASE_WORKSPACE_BYTES. */
enum { CU2REC_EASE_MAX_ITEMS = 65536, CU2REC_EASE_MAX_K = 256, CU2REC_EASE_WORKSPACE_BYTES = 64 << 20 };
typedef struct cu2rec_ease cu2rec_ease;
/* builds the model: G, its inverse and B, all in one buffer */
int cu2rec_ease_create(const cu2rec_csr *train, float l2, cu2rec_ease **out);
void cu2rec_ease_destroy(cu2rec_ease *ease);
int cu2rec_ease_info(const cu2rec_ease *ease, int *items, float *l2); /* pointers may be NULL */
/* items per block of the factorisation and the inverse (a constant of the build; needs no device) */
int cu2rec_ease_block_items(void);
/* G alone, dense -> out (host, I x I floats) */
int cu2rec_csr_ease_gram(const cu2rec_csr *csr, float l2, float *out);
/* rows of B (ids: host, duplicates allowed; NULL: every item, n ignored) -> out (host, n x I floats) */
int cu2rec_ease_weights(const cu2rec_ease *ease, const int *ids, int n, float *out);
/* the k largest B_ij, j != i, of each listed item i (ids as above) -> host, n x k */
int cu2rec_ease_neighbors(const cu2rec_ease *ease, const int *ids, int n, int k, int *out_ids, float *out_vals);
/* the k best candidates of each listed history row (users: host row ids of `history`, duplicates allowed; NULL: every row; row u
 * of `exclude` -- may be NULL, rows past its last exclude nothing -- is not listed for row u) -> host, n x k */
int cu2rec_ease_recommend(const cu2rec_ease *ease, const cu2rec_csr *history, const cu2rec_csr *exclude, const int *users, int n,
                          int k, int *out_items, float *out_scores);
/* cu2rec_model_rank_metrics' definitions over cu2rec_ease_recommend's lists of every history row (the rows the means are taken
 * over; test rows past them: CU2REC_EINVAL).  per_user: host, history rows x 5, may be NULL. */
int cu2rec_ease_rank_metrics(const cu2rec_ease *ease, const cu2rec_csr *history, const cu2rec_csr *exclude, const cu2rec_csr *test,
                             int k, float threshold, cu2rec_rank_metrics *out, double *per_user);

/* ------------------------------------------------------------------------------------------
 * SLIM (Ning & Karypis, "SLIM: Sparse Linear Methods for Top-N Recommender Systems", ICDM 2011): EASE's least-squares problem with an
 * L1 penalty and, optionally, non-negative weights; a weight matrix of a few per cent nonzeros.  With A = G of EASE above (X^T X with
 * l2 on the diagonal), column j of W minimises over w, with w_j = 0 and, when `positive`, w >= 0,
 *     1/2 w^T A w - sum_{k != j} A_kj w_k + l1 |w|_1.
 * EASE is l1 = 0 with free signs, at convergence.  The solver is cyclic coordinate descent from W = 0, in float32.  One sweep visits
 * the coordinates k = 0 .. I - 1 in ascending order, each for all columns j at once; with C = A - A W,
 *     rho = fmaf(A_kk, W_kj, C_kj);  new = max(rho - l1, 0) / A_kk when positive, else sign(rho) max(|rho| - l1, 0) / A_kk;
 *     new = 0 for k = j;  delta = new - W_kj;  W_kj = new;  C[:, j] -= delta A[:, k].
 * The device takes the coordinates in blocks of cu2rec_ease_block_items(): inside a block each delta reaches the block's later
 * coordinates as c = fmaf(-delta, A_sk, c) on a copy of C's rows, and after the block C -= A[:, block] Delta as one matrix-core tile
 * product per tile, from zero, subtracted with one rounding per element -- the same sequence of values as coordinate by coordinate,
 * up to float rounding.  A tile of Delta that is all zeros is skipped: the update it would make is an exact zero.
 *
 * At most max_sweeps sweeps are run; with tol > 0 a sweep whose largest |delta| is <= tol is the last (tol = 0: every sweep
 * is run).  report (may be NULL): the sweeps run, the last sweep's largest |delta|, the nonzeros of W.  No float atomics and a
 * fixed order of every sum: a model built twice is bit-identical.
 *
 * The handle is a cu2rec_ease: cu2rec_ease_weights (rows of W), cu2rec_ease_neighbors, cu2rec_ease_recommend (the score of a history
 * row for item j is sum_i r_ui W_ij, EASE's fold), cu2rec_ease_rank_metrics, cu2rec_ease_info (items and SLIM's l2) and
 * cu2rec_ease_destroy serve it as they serve EASE's B.
 *
 * Limits are EASE's: one GPU, I <= CU2REC_EASE_MAX_ITEMS (more: CU2REC_EUNSUPPORTED before anything is allocated).  While it is built
 * the model holds THREE (I rounded up to whole blocks)^2 float matrices (A, C and W) and afterwards one; memory that is not there is
 * CU2REC_ENOMEM.  l1 not finite or < 0, l2 not finite or <= 0, max_sweeps < 1, tol NaN or < 0, null arguments and a train row that
 * stores a column twice are CU2REC_EINVAL before anything is allocated.  A weight that is not a finite number (a NaN or an infinite
 * value in the data) fails the build with CU2REC_EUNSUPPORTED.  cols == 0 or nnz == 0 is a valid model of zeros. */
typedef struct { int sweeps; float last_delta; long long nonzeros; } cu2rec_slim_report;
int cu2rec_slim_create(const cu2rec_csr *train, float l1, float l2, int positive, int max_sweeps, float tol,
                       cu2rec_slim_report *report /* may be NULL */, cu2rec_ease **out);

/* ------------------------------------------------------------------------------------------
 * PureSVD (Cremonesi, Koren, Turrin, "Performance of Recommender Algorithms on Top-N Recommendation Tasks", RecSys 2010): the rank-f
 * truncated SVD of the rating matrix, scored as X Q Q^T.  The only training-free baseline that is a FACTOR model: its result is a
 * (P, Q) pair that cu2rec_model_topk, cu2rec_model_rank_metrics, cu2rec_model_similar, cu2rec_model_top_users, the five files and
 * bin/predict serve unchanged.  No learning rate, no regulariser, no seed beyond the start.
 *
 * X is the users x items matrix of the values `train` stores, entries that repeat a column within a row summed; f = n_factors.  Block
 * subspace (orthogonal) iteration from Q = the model's current item factors (a fresh model: initialize_normal_array, seed 42):
 *     each sweep:  Y = orth(X Q)   Q = orth(X^T Y)        at the end:  P = X Q,  user_bias = item_bias = 0
 * orth is Cholesky-QR applied twice; one pass forms G = Y^T Y, factors G = L L^T and sets Y <- Y L^-T, all in float32.  The scores
 * P Q^T depend only on the subspace Q spans, so there are no singular values, no ordering of the factors and no Rayleigh-Ritz step;
 * orthonormalising after every single multiply keeps cond(G) at (sigma_1 / sigma_f)^2.  Scores are p . q exactly only with a model
 * whose global_bias is 0 (cu2rec_train_svd insists on it; cu2rec_model_svd does not touch the model's).
 *
 * A pivot of a factorisation that is not a finite number above 2^-22 of its own diagonal entry (EASE's rule: f above the numerical
 * rank, a zero matrix, a NaN value) fails the call with CU2REC_EUNSUPPORTED, cu2rec_last_error() naming the sweep, the product and the
 * column.  The sweeps run in scratch buffers and the model is written at the end: a call that fails leaves P, Q and both biases bit
 * for bit as they were.  The host reads one status word per pass of orth: four stream synchronisations per sweep.
 *
 * Limits: one GPU; f <= CU2REC_ALS_MAX_FACTORS, train's rows >= f and cols >= f (else CU2REC_EUNSUPPORTED); sweeps >= 1, train within
 * the model's shape, non-null m / train (else CU2REC_EINVAL); all checked before the device or the model is touched.  Rows of the
 * model outside train's shape become zero rows.
 *
 * No float atomics; the order of every sum is a function of the row's length and f alone (rows longer than CU2REC_ALS_CHUNK are cut
 * by the ALS row plan, the chunks added in chunk order): a model built twice is bit-identical, and since Q is the only state that is
 * carried, sweeps = 2 twice is sweeps = 4 once, bit for bit.
 *
 * report (may be NULL): the sweeps run, captured = |X Q|_F^2 = |P|_F^2 and total = |X|_F^2, both summed in double in a fixed order;
 * captured / total is the share of the matrix's energy the subspace holds (at most 1 up to float rounding). */
typedef struct { int sweeps; double captured; double total; } cu2rec_svd_report;
int cu2rec_model_svd(cu2rec_model *m, const cu2rec_csr *train, int sweeps, cu2rec_svd_report *report /* may be NULL */);
/* out = H Q (host, history rows x n_factors, dense): the fold-in of new users by projection, p = r Q, for any CSR with the model's
 * column count (another: CU2REC_EINVAL).  The kernel and the row strides are cu2rec_model_svd's last product: projecting the training
 * matrix gives the model's P bit for bit.  The model is only read. */
int cu2rec_model_project(cu2rec_model *m, const cu2rec_csr *history, float *out);
/* PureSVD as a trainer, beside cu2rec_train_implicit: cfg->total_iterations sweeps of cu2rec_model_svd on `model`, whose n_factors must
 * be cfg->n_factors and whose global_bias must be 0 (else CU2REC_EINVAL).  The start is the model's item factors -- a fresh model's are
 * the seed-42 draw; a cfg->seed other than 42 first draws them again, initialize_normal_array(cols x f, f, seed).  Everything else in
 * cfg is ignored; cfg->cur_iterations advances by the sweeps.  verbose: one line,
 * "SVD: Factors: %d Sweeps: %d Captured: %f Total: %f Share: %f". */
int cu2rec_train_svd(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, int verbose, cu2rec_svd_report *report);
/* The two stages alone, for tests and tools.
 * cu2rec_csr_multiply: out[row, 0 : f] = sum over the row's entries of r * D[column, 0 : f] for every row of csr (transpose != 0: of
 * its item-major view, out = X^T D).  D: host, dense, (transpose ? rows : cols) x f.  It is staged at the model's row strides -- the
 * user side's rows at f rounded up to 4 floats, the item side's at f rounded up to 32, the padding filled with NaNs -- and out
 * (host) receives the PADDED rows as the device wrote them: (transpose ? cols : rows) x cu2rec_csr_multiply_stride(transpose, f)
 * floats, the padding columns zero.  f outside [1, CU2REC_ALS_MAX_FACTORS]: CU2REC_EUNSUPPORTED. */
int cu2rec_csr_multiply(const cu2rec_csr *csr, int transpose, const float *D, int f, float *out);
int cu2rec_csr_multiply_stride(int transpose, int f);
/* cu2rec_orthonormalize: Y (host, n x f, dense) <- orth(Y) in place.  A refused pivot is CU2REC_EUNSUPPORTED with *bad_column (may be
 * NULL; -1 otherwise) its column and Y untouched; n < f is refused before the device with column n. */
int cu2rec_orthonormalize(float *Y, int n, int f, int *bad_column);

#ifdef __cplusplus
}
#endif
#endif /* CU2REC_AMD_H */
