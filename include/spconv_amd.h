/* spconv_amd -- C ABI of the MI355X (gfx950) sparse-convolution hot path.
 *
 * This header is the drop-in boundary: every entry point takes plain device
 * pointers, sizes and a HIP stream (no torch / tensorview types) and replaces
 * one native call that traveller59/spconv's Python layer makes into its
 * pybind module `spconv.core_cc` (classes SpconvOps / ConvGemmOps, signatures in
 * spconv/core_cc/csrc/sparse/all/__init__.pyi and convops/spops.pyi).  The
 * reference interface each function replaces is cited as file:line relative to
 * the reference tree.  INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *  - All pointers are DEVICE pointers unless the name ends in `_h` (host).
 *  - All functions return 0 on success and a negative value on error; the
 *    message is available from spx_last_error() (thread local).  This replaces
 *    the C++ exceptions TV_ASSERT_RT_ERR / TV_THROW_RT_ERR of the reference.
 *  - No function allocates device memory: outputs and scratch ("ws") are
 *    supplied by the caller, exactly like the reference's ExternalAllocator
 *    contract (spconv/csrc/sparse/alloc.py:38-189, pytorch/cppcore.py:112-223).
 *    spx_*_ws_bytes() give the required scratch size (cf. all.py:1580-1605).
 *  - Work is enqueued on `stream` (a hipStream_t passed as void*; the reference
 *    passes the CUDA stream as an integer, pytorch/cppcore.py:98-99).  Nothing
 *    synchronises except spx_conv_rulebook_count (one D->H read of N_out, the
 *    same unavoidable read as indices.py:1454-1455).
 *  - indices: int32 [N, ndim+1] rows (batch, z, y, x), 1 <= ndim <= 4
 *    (pytorch/core.py:148,163).  Offsets are numbered k = (r0*K1 + r1)*K2 + r2,
 *    last spatial dim fastest (indices.py:114-136).
 *  - weight: KRSC [K, *ksize, C] contiguous (pytorch/conv.py:136-139).
 */
#ifndef SPCONV_AMD_H_
#define SPCONV_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPX_MAX_NDIM 4
#define SPX_UNION_MAX_OPERANDS 8   /* operands of one misaligned add (spx_union_*) */
/* reduction of an axis collapse (spx_collapse_fwd / _bwd) */
#define SPX_COLLAPSE_SUM 0
#define SPX_COLLAPSE_MEAN 1
#define SPX_COLLAPSE_MAX 2
/* row score of a voxel pruning step (spx_row_score) */
#define SPX_SCORE_ABSMEAN 0
#define SPX_SCORE_ABSMAX 1

typedef void *spx_stream_t; /* hipStream_t */

/* SPX_F64: float64 tensors of spx_igemm_fwd / _fwd_stats / _dgrad / _wgrad / _bwd, spx_bias_act_inplace and the four
 * pooling entries.  Their own kernels (csrc/igemm_f64.hip: v_mfma_f64_16x16x4_f64, float64 accumulation throughout) take
 * any channel count, any kernel volume in one launch and every table form, and need no scratch except the weight
 * gradient's (spx_igemm_wgrad_ws_bytes_dtype). */
enum spx_dtype { SPX_F32 = 0, SPX_F16 = 1, SPX_BF16 = 2, SPX_I8 = 3, SPX_F64 = 4 };

/* tv::gemm::Activation subset used by the path (csrc/sparse/inference.py:26-146) */
enum spx_act { SPX_ACT_NONE = 0, SPX_ACT_RELU = 1, SPX_ACT_SIGMOID = 2, SPX_ACT_LEAKY_RELU = 3 };
/* OR-ed into the `act` argument of spx_igemm_fwd: the result rows are stored with the default cache
 * policy instead of non-temporally.  For a layer whose output the NEXT launch reads (a BatchNorm right
 * behind the convolution): it then finds the rows in the caches (config 4: 3.54 -> 3.49 ms of kernels per
 * step).  Without it the rows leave the L2 as they are written, which is what a layer measured alone
 * wants (config 2: 37.4 -> 33.6 us per step). */
#define SPX_OUT_CACHED 0x100
/* OR-ed into the `act` argument of spx_igemm_fwd_int8 (which has no tile_order argument of its own):
 * `pair` and `mask` are stored in tile order, i.e. row t of the tables belongs to output row
 * argsort[t] (spx_permute_tables), as for tile_order = 1 of spx_igemm_fwd. */
#define SPX_TILE_ORDER 0x200

/* Error text of the last failing call on this thread ("" if none). */
const char *spx_last_error(void);

/* Library ABI version (major*1000 + minor). */
int spx_version(void);

/* Run-time override of a kernel-selection switch (same names as the SPX_* environment variables the
 * library reads, e.g. "SPX_CONV_V" = 2 | 3: generation of the strided-conv rulebook passes).  Stands in for the
 * per-process tuner state of the reference (ConvTunerSimple, csrc/sparse/convops.py:919-1466): tests and
 * the benchmark use it to run two kernel generations against each other inside one process.  Host only. */
int spx_set_option(const char *name_h, int value);

/* Diagnostics: how many launches of a kernel family this process has enqueued (or captured) so far -- "igemm_v4" (128 /
 * 64-row gather-GEMM tiles), "igemm_ws" (weight-stationary 512-row workgroups of dense C = K = 64 layers),
 * "igemm_v4w" (column-blocked launches of layers wider than 256 channels), "igemm_bwd" (fused dgrad + wgrad launch),
 * "igemm_bwd_rows" (one-gather backward), "igemm_i8_stream", "generic";
 * -1 for an unknown name.  The role of the reference's tuner record (which algorithm a layer was given:
 * ConvTunerSimple, csrc/sparse/convops.py:919-1466): lets a test or a benchmark say which kernel a call REALLY took
 * when the choice depends on an asynchronously read density class.
 * Keys with a '/' count one template INSTANCE (dt: f16 | bf16 | i8 | f32):
 *   igemm_v4/<COUT>/<MB>/<dt>/<fwd|bt>/<NKS>/<PK>   forward / dgrad gather-GEMM tile (bt: transposed weight reads)
 *   igemm_v4w/128/<dt>/<fwd|bt>/<NKS>/<PK>          the same, column-blocked (output widths beyond 256: 128-column x
 *                                                  64-row tiles; PK in {1, 2, 4}, PK > 1 with NKS 1 and a 16-bit dt; i8: fwd)
 *   igemm_bwd/<COUT>/<MB>/<dt>/<NKS>/<PK>           fused dgrad + wgrad launch
 *   igemm_ws/<dt>                                  weight-stationary kernel (forward and dgrad)
 *   igemm_bwd_rows/<C>/<K>/<dt>/<W8>               rows walk of narrow layers (W8: 0 | 1, eight waves)
 *   wgrad_tr/<dt>/<SL>, wgrad_f32                  weight gradient, first stage (SL: 2 | 4 | 8 live slots per row)
 *   wgrad_mfma/<dt>, wgrad_generic/<dt>            weight gradient, fallback kernels
 *   generic/<dt>, gen1/<COUT>/<dt>                 one-thread-per-output and first-generation gather-GEMM
 *   sparse_hint/v4, sparse_hint/bwd                igemm_v4 (forward, dgrad) / igemm_bwd launches whose appendix part was
 *                                                  shaped by SPX_SPARSE_ROWS_HINT (counted next to their family)
 *   dense/map, dense/scatter_cl, dense/scatter_cf, dense/gather_cl, dense/gather_cf, dense/compact
 *                                                  sparse <-> dense conversion (cl / cf: channels last / first)
 *   union/mark, union/prefix, union/claim, union/fill, union/add_fwd, union/add_bwd
 *                                                  misaligned add: the stages of the union build (prefix: the prefix
 *                                                  pass and its block scan, counted once) and the two merge launches
 *   collapse/mark, collapse/prefix, collapse/rank, collapse/list, collapse/fwd, collapse/bwd
 *                                                  axis collapse: the passes of the build (prefix: the prefix pass and
 *                                                  its block scan; list: the radix argsort and the boundary launch
 *                                                  behind it, counted once) and the two reduction launches
 *   pointvoxel/groups, pointvoxel/gather, pointvoxel/decorate
 *                                                  point <-> voxel features: calls of spx_point_groups (the key pass, the
 *                                                  radix argsort and the boundary launch, counted once),
 *                                                  spx_voxel_to_point and spx_point_decorate
 *   interp/corners_ranked, interp/corners_hash, interp/fwd, interp/bwd
 *                                                  trilinear devoxelisation: calls of spx_point_corners by lookup form,
 *                                                  of spx_interp_fwd and of spx_interp_bwd
 *   query/ranked, query/hash, query/group_fwd, query/group_bwd
 *                                                  voxel query and grouping: calls of spx_voxel_query by lookup form,
 *                                                  of spx_group_fwd and of spx_group_bwd
 *   sample/fps, sample/ball_query, sample/knn_query
 *                                                  raw-point sampling: calls of spx_fps, of spx_ball_query and of
 *                                                  spx_knn_query that launch
 *   select/score, select/hist, select/pick, select/ties, select/flags, select/count, select/scan, select/scatter,
 *   select/map                                     voxel pruning, one count per launch: spx_row_score; the passes of
 *                                                  spx_topk_flags (hist and pick once per 8-bit digit: four each; ties:
 *                                                  the blocks' tie counts and their scan, counted once); the passes of a
 *                                                  selection build (map: spx_rankmap_from_sorted over the result)
 *   box/corners, box/pairs, box/aligned, box/key, box/mask, box/reduce
 *                                                  rotated boxes, one count per launch: spx_boxes_to_corners,
 *                                                  spx_boxes_overlap, spx_boxes_overlap_aligned and the three kernels
 *                                                  of spx_nms_rotated (its sort counts under serialize/sort)
 *   serialize/keys, serialize/sort, serialize/offsets, serialize/plan, serialize/bwd
 *                                                  voxel serialisation: calls of spx_curve_keys; sorted orders of
 *                                                  spx_serialize (one per key row, none for n = 0); its offsets launch;
 *                                                  calls of spx_patch_plan and of spx_patch_rows_bwd
 * COUT in {16, 32, 64, 128, 256}, NKS in {1, 2}, PK in {1, 2, 4, 8, 16, 32}.  A well-formed key of an instance that is
 * never built counts 0; anything else is unknown.
 * float64 (SPX_F64) has a family and keys of its own, outside the dt vocabulary above:
 *   igemm_f64                                      every float64 gather-GEMM launch (forward and dgrad)
 *   igemm_f64/fwd, igemm_f64/dgrad                 the same, by role
 *   wgrad_f64                                      float64 weight gradient, first stage
 *   pool/f64                                       float64 pooling (max / avg, forward / backward)
 * Pooling (pool.hip) counts every kernel instance, float64 included:
 *   pool/<op>/<dt>/<piece>                         op: max_fwd | max_bwd | avg_fwd | avg_bwd; dt: f16 | bf16 | f32 | f64 |
 *                                                  i8; piece: v (16-byte pieces, C a multiple of 16 / sizeof(dt)) | s (one
 *                                                  element per thread).  int8 exists for max_fwd only: 34 instances.
 * The rulebook builders over the hash table (spx_subm_rulebook, spx_conv_rulebook_count / _fill / _static) count every
 * dispatch decision of a build, where the launch is issued:
 *   rulebook/subm_probe3 | subm_probe4 | subm_probe5  form of the SubM probe pass (probe3: kernel volume 1, beyond 128,
 *                                                  or more than 4 M voxels; probe5: tables of 2^10 .. 2^19 slots)
 *   rulebook/subm_mask_pass                        SubM masks from a pass over the finished table (SPX_SUBM_MASK_PASS)
 *   rulebook/subm_lists, rulebook/native_lists_v1  SubM Native lists from the probe's group counts / by count -> scan ->
 *                                                  scatter (behind subm_probe3)
 *   rulebook/conv3/<MJ>, rulebook/conv_generic     strided convolution: compact-candidate passes (MJ in {1, 2, 4, 8}
 *                                                  candidates per input) / one thread per (offset, input) (SPX_CONV_V = 2,
 *                                                  transposed, stride 1, ...); once per count pass and once per fill pass
 *   rulebook/conv_lists_v1                         strided-convolution lists by count -> scan -> scatter (kernel volume
 *                                                  beyond 128)
 *   rulebook/conv_shrunk, rulebook/conv_retry      count pass over a table sized for the outputs expected (last ratio /
 *                                                  static bound); count pass run again at the guaranteed size after that
 *                                                  table overflowed
 *   rulebook/conv3_shares/<S>                      grid.y of the compact-candidate passes (S in {1, 2, 4, 8} shares per
 *                                                  input row; SPX_TEST_CONV3_SHARES), once per count pass and once per
 *                                                  fill pass
 * Host only. */
long long spx_launch_count(const char *family_h);

/* dst[r] = src[r] followed by zeros: rows of src_row_bytes bytes widened to dst_row_bytes (both even), one launch.  The
 * channel padding of layers whose widths the MFMA kernels are not instantiated for (the 3-5 channel first layer of a
 * voxel backbone: the reference pads nothing and tunes a kernel per shape, csrc/sparse/convops.py:919-1466). */
int spx_pad_rows(const void *src, void *dst, long long rows, int src_row_bytes, int dst_row_bytes,
                 spx_stream_t stream);

/* ops.get_conv_output_size / get_deconv_output_size (pytorch/ops.py:73-96). Host only. */
int spx_conv_out_shape(int ndim, const int *in_shape, const int *ksize, const int *stride,
                       const int *padding, const int *dilation, const int *out_padding,
                       int transposed, int *out_shape);

/* ------------------------------------------------------------------ rulebook */

/* Scratch bytes for spx_subm_rulebook (hash table + compaction counters). */
size_t spx_subm_rulebook_ws_bytes(int n, int kv);

/* SubM rulebook.  Replaces SpconvOps.generate_subm_conv_inds[_cpu]
 * (csrc/sparse/indices.py:1495-1599 GPU, :1639-1708 CPU; drivers all.py:628-660,
 * pytorch/ops.py:202-233,505-565).
 *   pair_fwd  [kv, n]  out: pair_fwd[k][o] = input index feeding output o through
 *                      offset k, or -1 (implicit-GEMM layout, indices.py:806-874)
 *   pair_bwd  [kv, n]  or NULL: pair_bwd[k][i] = output index fed by input i
 *   mask      [n, ceil(kv/32)] uint32: bit k set iff pair_fwd[k][o] >= 0
 *                      (centre bit always set, indices.py:1576-1577)
 *   pair_native [2, kv, n] or NULL: ConvAlgo.Native lists, identical (including
 *                      order and -1 fill) to the CPU path indices.py:1639-1708
 *   num_per_loc [kv]   or NULL: counts for k < kv/2 only, like the CPU path
 * Duplicate coordinates: the smallest index wins (CPU unordered_map::insert). */
int spx_subm_rulebook(const int32_t *indices, int n, int ndim, int batch_size,
                      const int *spatial_shape, const int *ksize, const int *dilation,
                      int32_t *pair_fwd, int32_t *pair_bwd, uint32_t *mask,
                      int32_t *pair_native, int32_t *num_per_loc,
                      void *ws, size_t ws_bytes, spx_stream_t stream);

/* Scratch bytes for the two-phase regular/transposed conv rulebook.  The output hash table is
 * sized for N * prod_i ceil(k_i * gcd(d_i, s_i) / s_i) distinct outputs (kv * N when transposed):
 * SpconvOps.get_handcrafted_max_act_out (all.py:1557-1578) with dilation taken into account;
 * `dilation` may be NULL (= all ones).  spx_conv_rulebook_count fails loudly if the bound is
 * ever exceeded. */
size_t spx_conv_rulebook_ws_bytes(int n_in, int ndim, const int *ksize, const int *stride,
                                  const int *dilation, int transposed);

/* Regular / transposed conv rulebook, phase 1: hash the candidate output
 * coordinates and count the distinct ones.  Replaces stage1 + unique
 * (indices.py:501-597,997-1016,1118-1455; pytorch/ops.py:566-642).
 * Writes the count to *n_out_h after synchronising `stream` (the one D->H read); with
 * n_out_h == NULL nothing is read and the count stays in the workspace (spx_conv_rulebook_static).
 * `ws` must be passed unchanged to spx_conv_rulebook_fill. */
int spx_conv_rulebook_count(const int32_t *indices, int n_in, int ndim, int batch_size,
                            const int *in_shape, const int *out_shape, const int *ksize,
                            const int *stride, const int *padding, const int *dilation,
                            int transposed, void *ws, size_t ws_bytes, int *n_out_h,
                            spx_stream_t stream);

/* Phase 2: number the outputs in the CPU path's first-seen order (k-major,
 * then input-major, indices.py:1742-1771) and fill every artefact.  Replaces
 * assign_output + stage2 (indices.py:417-499,599-721; ops.py:646-714).
 *   out_indices [n_out, ndim+1]
 *   pair_fwd [kv, n_out], pair_bwd [kv, n_in]  (-1 = absent)
 *   mask_fwd [n_out, W], mask_bwd [n_in, W] (or NULL)
 *   pair_native [2, kv, n_in] (or NULL), num_per_loc [kv] (or NULL): identical
 *   to SparseConvIndicesCPU::generate_conv_inds (indices.py:1710-1778). */
int spx_conv_rulebook_fill(const int32_t *indices, int n_in, int ndim, int batch_size,
                           const int *in_shape, const int *out_shape, const int *ksize,
                           const int *stride, const int *padding, const int *dilation,
                           int transposed, int n_out, int32_t *out_indices,
                           int32_t *pair_fwd, int32_t *pair_bwd, uint32_t *mask_fwd,
                           uint32_t *mask_bwd, int32_t *pair_native, int32_t *num_per_loc,
                           void *ws, size_t ws_bytes, spx_stream_t stream);

/* Static-shape form of the two phases above: room for n_out_cap outputs, NOTHING read back, every
 * launch stream-ordered -- the call can be captured in a hipGraph and replayed on new coordinates of
 * the same n_in.  It is the GPU side of the reference's bounded inference mode (num_out_act_bound,
 * ops.py:263-266,644-645; the pre-sized workspace of csrc/sparse/all.py:2030-2185).
 *   - input rows with batch index < 0 are dead rows (padding up to the static n_in): they create no
 *     output and no pair
 *   - outputs are numbered in the CPU path's first-seen order; the first n_out_cap survive, pairs
 *     into later ones are dropped (as with spx_conv_rulebook_fill and n_out < the count)
 *   - out_indices rows past the number of outputs are -1 (dead rows for the next layer), their
 *     pair_fwd column is -1 and their mask 0
 *   - pair_native / num_per_loc (or NULL): the ConvAlgo.Native lists as spx_conv_rulebook_fill writes
 *     them (training: the weight-gradient kernels read them); dead rows are in no list
 *   - n_out_dev [2] (device): {distinct outputs found -- may exceed n_out_cap --, hash-table
 *     overflow flag: more distinct candidates than the table sized for 2 x n_out_cap holds};
 *     the caller reads it whenever it next synchronises
 * spx_conv_rulebook_count with n_out_h == NULL is the same count without the read. */
int spx_conv_rulebook_static(const int32_t *indices, int n_in, int ndim, int batch_size,
                             const int *in_shape, const int *out_shape, const int *ksize,
                             const int *stride, const int *padding, const int *dilation,
                             int transposed, int n_out_cap, int32_t *out_indices,
                             int32_t *pair_fwd, int32_t *pair_bwd, uint32_t *mask_fwd,
                             uint32_t *mask_bwd, int32_t *pair_native, int32_t *num_per_loc,
                             int32_t *n_out_dev, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ---- sorted-order levels ---------------------------------------------------------------------------
 * The reference's GPU path does not fix the order of a strided convolution's outputs: they come out of a
 * sort + unique of the linear coordinate keys (csrc/sparse/all.py:1533-1552 apply_thrust_unique_to_indice_pairs_uniq)
 * or out of a hash table in slot order (csrc/sparse/indices.py:1380-1425); only the CPU path is first-seen
 * (indices.py:1742-1771, what spx_conv_rulebook_fill reproduces).  The calls below produce the SORTED order
 * (batch-major linear key, last spatial dimension fastest) without a sort and without a hash table, through the
 * RANK MAP of the output level: one {occupancy bits, number of occupied cells before the word} pair per 32
 * consecutive keys (the prefix counted inside a block of 2048 words, the blocks' own offsets behind the words); row of a
 * key = block offset + prefix + popcount of the bits below it.  (Built from a byte per cell in the workspace -- plain
 * idempotent stores, no atomics -- that a prefix pass packs into the words.)  The map is the caller's buffer
 * (spx_rankmap_bytes; 0 = key space beyond 2^31 cells: keep the hash builder) and stays valid after the call:
 * spx_subm_rulebook_ranked builds the SubM rulebook of a layer BEHIND the strided one from it -- no table fill,
 * no insert, one 8-byte load per neighbour query.  Rows in key order put x-neighbours in adjacent rows, which is
 * what the gather kernels of the level gain (tools/order_probe.py).
 * Values per coordinate are those of the first-seen build; only the row numbering differs.
 * spx_conv_sorted_ok: 1 when the geometry has compact candidates (at most 8 per input and at most half of the
 * offsets: k3 s2, k2 s2, k3 s3, ...; not transposed, not stride 1, not (3,1,1)/(2,1,1)) and the key space fits. */
size_t spx_rankmap_bytes(int ndim, int batch_size, const int *shape);
int spx_conv_sorted_ok(int ndim, int batch_size, const int *in_shape, const int *out_shape, const int *ksize,
                       const int *stride, const int *padding, const int *dilation, int transposed);
size_t spx_conv_rulebook_sorted_ws_bytes(int n_in, int ndim, int batch_size, const int *out_shape,
                                         const int *ksize);
/* phase 1 (as spx_conv_rulebook_count: the one D->H read of the count), phase 2 (as spx_conv_rulebook_fill)
 * and the static-shape form (as spx_conv_rulebook_static, with n_out_dev [3]: {outputs found, 0 -- a rank map cannot
 * overflow --, live output rows = min(found, n_out_cap)}).
 * `rankmap` and `ws` must be passed unchanged from phase 1 to phase 2. */
int spx_conv_rulebook_count_sorted(const int32_t *indices, int n_in, int ndim, int batch_size,
                                   const int *in_shape, const int *out_shape, const int *ksize,
                                   const int *stride, const int *padding, const int *dilation,
                                   void *rankmap, size_t rankmap_bytes, void *ws, size_t ws_bytes,
                                   int *n_out_h, spx_stream_t stream);
int spx_conv_rulebook_fill_sorted(const int32_t *indices, int n_in, int ndim, int batch_size,
                                  const int *in_shape, const int *out_shape, const int *ksize,
                                  const int *stride, const int *padding, const int *dilation, int n_out,
                                  int32_t *out_indices, int32_t *pair_fwd, int32_t *pair_bwd,
                                  uint32_t *mask_fwd, uint32_t *mask_bwd, int32_t *pair_native,
                                  int32_t *num_per_loc, void *rankmap, size_t rankmap_bytes, void *ws,
                                  size_t ws_bytes, spx_stream_t stream);
int spx_conv_rulebook_static_sorted(const int32_t *indices, int n_in, int ndim, int batch_size,
                                    const int *in_shape, const int *out_shape, const int *ksize,
                                    const int *stride, const int *padding, const int *dilation,
                                    int n_out_cap, int32_t *out_indices, int32_t *pair_fwd,
                                    int32_t *pair_bwd, uint32_t *mask_fwd, uint32_t *mask_bwd,
                                    int32_t *pair_native, int32_t *num_per_loc, int32_t *n_out_dev,
                                    void *rankmap, size_t rankmap_bytes, void *ws, size_t ws_bytes,
                                    spx_stream_t stream);
/* The rank map of a level whose rows ALREADY are in ascending, unique key order -- level 1 of a backbone whose data
 * loader sorts the voxels it hands over (the reference's own GPU builders emit such rows for every strided level:
 * csrc/sparse/all.py:1533-1552; its voxelisers emit point / hash-slot order, pytorch/utils.py:23-160).  Row = rank:
 * two launches (a fill of the map, one pass over the rows), no marks, no scan, no atomics.  `violation` (device
 * int32 [1], or NULL) is set to 1 when a live row's key is not above its predecessor's or a live row follows a dead
 * one (batch -1 rows must trail); the caller decides when to read it.  With the map attached, the level's SubM layers
 * take spx_subm_rulebook_ranked (no hash table) -- replaces, for such levels, the insert + probe passes of
 * csrc/sparse/indices.py:723-741,806-874. */
int spx_rankmap_from_sorted(const int32_t *indices, int n, int ndim, int batch_size, const int *spatial_shape,
                            void *rankmap, size_t rankmap_bytes, int32_t *violation, spx_stream_t stream);
/* Rows in key order when the caller's are not: order[t] = the row with the t-th smallest linear coordinate key
 * (batch-major, last axis fastest), rows that are dead (batch -1) or out of range behind every live row in their own
 * order; `indices_sorted` (or NULL) receives indices[order[t]] (dead rows: -1s).  The keys of a level are unique, so
 * this is four launches: one stable radix pass on the upper key bits (<= 511 buckets of 2^sh consecutive keys,
 * sh <= 20), then a workgroup per bucket ranks its rows through an occupancy bit per key in LDS -- nothing is compared.
 * A coordinate that occurs twice still yields a permutation (its extra rows land behind their bucket's distinct keys);
 * spx_rankmap_from_sorted raises its flag on such a result.  Nothing is read back (hipGraph-safe): a captured pass
 * sorts its scene at the entry (StaticInference / StaticTrainingStep entry_sort), hands spx_rankmap_from_sorted the
 * result and runs every level in key order.  With `rankmap` (spx_rankmap_bytes() bytes, or NULL) the bucket pass leaves
 * the rank map of indices_sorted behind as well -- what spx_rankmap_from_sorted would build from it; its fill rides
 * in the sort's first launch: no pass of its own -- and `violation` (device int32 [1] or NULL: cleared by the first launch) is
 * raised when a coordinate occurs twice.  `rows` / `rows_sorted` (or NULL; row_bytes a multiple of 4): rows that travel with
 * the sort -- the level's features -- rows_sorted[t] = rows[order[t]], written by the same bucket pass (no gather launch).
 * Needs batch x grid <= 0xffe00000.  The reference sorts keys where it
 * wants this order (thrust sort + unique of the output keys, csrc/sparse/all.py:1533-1552). */
size_t spx_key_argsort_ws_bytes(int n);
int spx_key_argsort(const int32_t *indices, int n, int ndim, int batch_size, const int *spatial_shape, int32_t *order,
                    int32_t *indices_sorted, void *rankmap, size_t rankmap_bytes, int32_t *violation, const void *rows,
                    void *rows_sorted, int row_bytes, void *ws, size_t ws_bytes, spx_stream_t stream);
/* SubM rulebook (outputs as spx_subm_rulebook, bit for bit) of a level whose rows are in key order and whose
 * rank map a sorted-order build left behind: `indices` must be that build's out_indices (rows past its count:
 * batch -1). */
size_t spx_subm_rulebook_ranked_ws_bytes(int n, int kv);
int spx_subm_rulebook_ranked(const int32_t *indices, int n, int ndim, int batch_size,
                             const int *spatial_shape, const int *ksize, const int *dilation,
                             int32_t *pair_fwd, int32_t *pair_bwd, uint32_t *mask,
                             int32_t *pair_native, int32_t *num_per_loc, const void *rankmap,
                             size_t rankmap_bytes, void *ws, size_t ws_bytes, spx_stream_t stream);

/* mask_argsort: permutation that groups rows with equal masks (stable, ascending
 * mask value).  Replaces SpconvOps.sort_1d_by_key_allocator (all.py:935-991). */
size_t spx_mask_argsort_ws_bytes(int n);
int spx_mask_argsort(const uint32_t *mask, int n, int words, int32_t *argsort,
                     void *ws, size_t ws_bytes, spx_stream_t stream);
/* The same sort when the caller knows the kernel volume: only the low kv bits of a mask word can be set, so the sort
 * runs ceil(kv / 9) or ceil(kv / 8) digit passes instead of four (27 offsets: three). */
int spx_mask_argsort_kv(const uint32_t *mask, int n, int kv, int32_t *argsort, void *ws, size_t ws_bytes,
                        spx_stream_t stream);

/* Layout conversions for callers that hold only one of the two rulebook forms
 * (the reference's public ops take either the Native lists, pytorch/ops.py:811-988,
 * or the dense tables, ops.py:1450-1896).
 *  spx_native_to_table: table[k][dst] = src for every list entry (dst/src = out/in,
 *     exchanged when inverse != 0); mask [n_dst, W] optional.
 *  spx_table_to_native: Native lists from pair_fwd (subm != 0, uses the mirror
 *     symmetry) or from pair_bwd [kv, n_in] (subm == 0); order as the CPU path. */
int spx_native_to_table(const int32_t *pair_native, const int32_t *num_per_loc, int n_in,
                        int n_dst, int kv, int subm, int inverse, int32_t *table,
                        uint32_t *mask, spx_stream_t stream);
size_t spx_table_to_native_ws_bytes(int n, int kv);
int spx_table_to_native(const int32_t *table, int subm, int kv, int n, int32_t *pair_native,
                        int32_t *num_per_loc, void *ws, size_t ws_bytes, spx_stream_t stream);

/* -------------------------------------------------------------- convolution */

/* Kernel volumes 33 .. 128 (the reference's multi-word masks, indices.py:1601-1618, ops.py:448,494-503)
 * run as ceil(kv / 32) launches of the MFMA kernel whose partial sums travel through an fp32
 * [n_dst, cout] scratch: pass spx_igemm_acc_bytes() bytes as `ws` to spx_igemm_fwd (n_dst = n_out,
 * cout = K) / spx_igemm_dgrad (n_dst = n_in, cout = C).  0 for kv <= 32; without the scratch such
 * layers take the generic (one thread per output) kernel.
 *
 * Output widths (K of spx_igemm_fwd / _stats / _int8, C of spx_igemm_dgrad and of the dgrad half of spx_igemm_bwd): the
 * MFMA kernels run 16 / 32 / 64 / 128 / 256 and, beyond 256, every multiple of 128 -- one column-blocked launch
 * (igemm_wide.hip) for every table form, with the scratch row stride the full width; tensors beyond its 32-bit buffer
 * offsets (2 GiB per operand) take the generic kernel at these widths, tables by row or a rows layout (there is no
 * first-generation instance beyond 256 columns).  Other widths take the generic
 * kernel (float) or are refused (int8): callers zero-pad (the Python drivers do).  The reduction side only has to be a
 * whole number of 16-byte lane pieces.  Launches beyond 256 columns leave no BatchNorm statistics
 * (spx_igemm_fwd_stats: *slots_used_h = 0), and the fused backward stays at C <= 128. */
size_t spx_igemm_acc_bytes(int n_dst, int cout, int kv);

/* What the gather-GEMM entries may be handed (spx_igemm_fwd / _fwd_stats / _fwd_int8 / _dgrad / _wgrad / _bwd / _bwd_rows /
 * _bwd_deferred + spx_wgrad_stage2_batch, spx_bias_act_inplace); tests/test_gpu_gemm_isolation.py holds every kernel family
 * to it:
 *   (a) Dirty memory on entry.  Outputs, workspaces and statistics records may hold any bytes on entry: every element the
 *       caller reads afterwards has been stored, no region of a workspace is read before it is written.
 *   (b) Rows that no pair names.  A feature row or dout row that no table column, list entry or identity offset names may
 *       hold anything, NaN and Inf included (the dead rows of a static-shape tensor are such rows); it changes no output
 *       bit.  An identity offset (identity_k >= 0; subm = 1 in the backward entries, whose centre list is the identity
 *       over all rows) NAMES every row: a caller with dead rows in a SubM layer keeps them finite, or passes
 *       identity_k = -1 / explicit lists and leaves them out of the tables.  spx_igemm_bwd_rows reads its whole table.
 *   (c) Row outputs.  An element of out / din is NaN, +Inf or -Inf exactly where the sum over the existing pairs is, and
 *       this holds through bias and activation with torch's semantics: relu(NaN) = NaN, relu(-Inf) = 0,
 *       sigmoid(+-Inf) = 1 / 0, leaky slope x Inf keeps its sign.  (The fused BatchNorm + ReLU apply of
 *       spx_batchnorm_fwd does the same.)
 *   (d) Weight gradient.  Every element that is non-finite in the sum over the listed pairs is non-finite in dW (nothing
 *       is swallowed).  A non-finite dW[kk, k, c] occurs only if some NAMED feat row is non-finite in channel c or some
 *       named dout row is non-finite in column kk.  It may occur at an offset k the sum itself is finite at: the row-tile
 *       form (spx_igemm_bwd_rows) multiplies a tile's feat rows with the zero row an absent pair gathers, 0 x Inf = NaN.
 *   (e) Non-finite weights, bias or int8 scales are outside the contract: MFMA tiles multiply absent pairs as zero rows. */

/* Output-stationary implicit GEMM (atomics-free):
 *   out[o,:] = sum_k [pair[k][o] >= 0] feat[pair[k][o],:] * W[:,k,:]^T  (+bias, act)
 * Replaces ConvGemmOps.implicit_gemm forward (csrc/sparse/convops.py:2073-2243,
 * pytorch/ops.py:1450-1664).
 *   feat [n_in, C], weight KRSC [K, kv, C], out [n_out, K]: all `dtype`
 *   pair [kv, n_out]; mask [n_out, W] or NULL; argsort [n_out] or NULL
 *   identity_k: offset whose pair is the identity (SubM centre, kv/2) or -1
 *   bias [K] (dtype) or NULL; act: spx_act (inference epilogue, conv.py:463-490)
 *   dtype: SPX_F32 / SPX_F16 / SPX_BF16 / SPX_F64 (float64: any C and K, any kv in one launch, ws unused; the
 *   SPX_OUT_CACHED and SPX_DENSE_HINT bits are accepted and ignored)
 * Every row of `out` is written (no pre-zeroing needed, cf. convops.py:2128-2134). */
int spx_igemm_fwd(const void *feat, const void *weight, void *out, const int32_t *pair,
                  const uint32_t *mask, const int32_t *argsort, int tile_order, int n_in, int n_out,
                  int C, int K, int kv, int dtype, int identity_k, const void *bias,
                  int act, float act_alpha, void *ws, size_t ws_bytes,
                  spx_stream_t stream);

/* The same launch, and the BatchNorm statistics of the rows it stores on the way out: workgroup b of the launch leaves
 * {rows, mean, M2 = sum of squared deviations} of every output channel at stats[field][channel][b], i.e. float
 * (field * K + channel) * records + b with records = *slots_used_h (fp32, field 0 rows / 1 mean / 2 M2; statistics of the
 * ROUNDED output values, i.e. of what a normalisation layer behind the convolution reads), rows >= *n_live (device,
 * static-shape tensors; NULL = every row) not counted.  *slots_used_h (host) = number of records written = the
 * launch's workgroup count, or 0 when the kernel that was dispatched leaves none (bias / activation in the epilogue,
 * kernel volumes > 32, widths beyond 256, generic kernels, SPX_F64): spx_batchnorm_fwd_stats then starts at its merge step instead of reading the
 * rows again for a statistics pass.  `stats` holds stats_slots >= spx_igemm_fwd_stats_slots(n_out) records.
 * The reference leaves BatchNorm to torch on the feature matrix (spconv/pytorch/modules.py:127-168): two extra passes
 * over every activation; this removes the first of them. */
int spx_igemm_fwd_stats_slots(int n_out);
int spx_igemm_fwd_stats(const void *feat, const void *weight, void *out, const int32_t *pair,
                        const uint32_t *mask, const int32_t *argsort, int tile_order, int n_in, int n_out, int C,
                        int K, int kv, int dtype, int identity_k, const void *bias, int act,
                        float act_alpha, void *ws, size_t ws_bytes, float *stats, int stats_slots,
                        const int32_t *n_live, int *slots_used_h, spx_stream_t stream);

/* int8 inference forward.  Replaces the int8 branch of ConvGemmOps.implicit_gemm
 * (pytorch/ops.py:1540-1553,1631-1662, csrc/sparse/convops.py:2176-2205) as driven by the
 * quantised module (pytorch/quantization/quantized/conv.py:368-378).  Numerics pinned by the
 * reference's numpy formula (test/test_all_algo.py:272-287):
 *   v = acc_i32 * scale[k] + bias[k] + add[o][k] * add_scale;  v = act(v)
 *   out_dtype SPX_I8: clip(round_half_even(v), -128, 127);  SPX_F16 / SPX_BF16 / SPX_F32: v
 *   feat int8 [n_in, C], weight int8 KRSC [K, kv, C], scale / bias fp32 [K] (or NULL = 1 / 0),
 *   add int8 [n_out, K] or NULL (the module passes add_scale = add_q_scale / output_scale).
 * C must be a multiple of 16, K one of 16/32/64/128/256 or a multiple of 128 beyond, kv <= 32 (the reference's int8 kernels
 * need C, K % 16 == 0 as well, test/test_all_algo.py:376-377). */
int spx_igemm_fwd_int8(const void *feat, const void *weight, void *out, const int32_t *pair,
                       const uint32_t *mask, const int32_t *argsort, int n_in, int n_out, int C,
                       int K, int kv, int identity_k, const float *scale, const float *bias,
                       const void *add, float add_scale, int out_dtype, int act, float act_alpha,
                       spx_stream_t stream);

/* Copies of a pair table [kv, n] and its mask words in TILE ORDER (row t <- row order[t], order =
 * spx_mask_argsort's output): with tile_order = 1, spx_igemm_fwd / _dgrad / _bwd read `pair` and
 * `mask` by tile position and use `argsort` only for the operand / output rows, so a mask-sorted
 * tile reads its table columns as contiguous runs.  (The reference reads its tables through
 * mask_argsort, ops.py:1503-1530.) */
int spx_permute_tables(const int32_t *pair, const uint32_t *mask, const int32_t *order, int kv, int n,
                       int words, int32_t *pair_t, uint32_t *mask_t, spx_stream_t stream);

/* ---- density-aware row layout: the DEFAULT row order of a SubM rulebook -----------------------
 * The reference sorts the rows of every rulebook by mask (SPCONV_DO_SORT = "1", constants.py:121;
 * pytorch/ops.py:346,550,763-785 -> SpconvOps.sort_1d_by_key_allocator, all.py:935-991) so that its
 * implicit-GEMM tiles skip the offsets none of their rows has.  spx_subm_layout does that job INSIDE
 * the rulebook build -- no sort, nothing read back: the masks of the finished tables are classified
 * on the device and, for a SPARSE rulebook (fewer than a quarter of the rows have any neighbour), the
 * rows WITH a neighbour are taken out of the row-order walk into a compact appendix, grouped by their
 * lowest neighbour offset (a stable counting partition: wave ballots + prefix sums).  The gather-GEMM
 * then runs the rows in their own order with the CENTRE pair only -- a plain streaming GEMM: no row
 * order to fetch, no pair word, one step per tile -- and a handful of appendix tiles with all their
 * offsets.  A DENSE rulebook (LiDAR) keeps everything in the row-order walk (regrouping loses there).
 * The result is ONE int32 blob (pass it as `argsort` with tile_order = SPX_ROWS_LAYOUT;
 * spx_igemm_fwd_int8: OR SPX_ROWS_LAYOUT_ACT into `act`; `pair` / `mask` stay the row-order tables):
 *   [0] class: 1 = appendix in use, 0 = none   [1] M = rows with a neighbour   [2] n   [3] kv   [4] mcap
 *   main mask  [npad]       row-order mask words; class 1: ZERO for the rows that moved to the appendix
 *                           (a zero mask word means: not this tile's row, nothing stored)
 *   order      [mcap]       appendix position -> row       (first M entries; class 1 only)
 *   mask       [mcap]       mask words of those rows
 *   pair       [kv, mcap]   their pair words
 *   npad = n rounded up to 64, mcap = spx_subm_layout_mcap(n) >= n / 4 + 256.
 * The launch is the same for both classes (hipGraph-safe): ceil(n / 4 / tile rows) appendix workgroups
 * lead the grid, read {class, M} and leave at once when there is nothing for them; the M rows are dealt to
 * them in whole 16-row blocks (ceil(M / workgroups) rows each, rounded up to 16), so that a short appendix
 * becomes many short tiles instead of a few long ones. */
size_t spx_subm_layout_mcap(int n);
#define SPX_ROWS_LAYOUT 2
/* OR-ed into `tile_order` of spx_igemm_fwd / spx_igemm_dgrad: the HOST knows that the rulebook's neighbourhoods are
 * dense (it has seen class word 0 of the rows layout, or knows its data).  C = K = 64 16-bit layers then take the
 * weight-stationary gather-GEMM (csrc/igemm_ws.hip: one 512-row workgroup per CU, weights staged nine offsets at a time
 * through LDS-DMA) instead of the 128-row tiles -- a launch SHAPE, which is why it cannot be read on the device.  Results
 * are bit-identical with and without the hint; a wrong hint only costs time.  Stands in for the reference's tuner choice
 * between implicit-GEMM tile shapes (spconv/csrc/sparse/convops.py:1150-1297). */
#define SPX_DENSE_HINT 0x100
/* OR-ed into `tile_order` of spx_igemm_fwd / _fwd_stats / _dgrad / _bwd / _bwd_deferred next to SPX_ROWS_LAYOUT: the
 * HOST has READ the header of THIS blob, its class word is 1, and bits 12..30 carry its word [1], the EXACT M:
 *   tile_order = SPX_ROWS_LAYOUT | SPX_SPARSE_ROWS_HINT | (M << SPX_SPARSE_ROWS_SHIFT),  0 <= M <= SPX_SPARSE_ROWS_MAX.
 * f16 / bf16 launches of up to 256 output columns then hold exactly the appendix workgroups that receive rows under
 * the dealing rule above (instead of the n / 4 rows' worth the class rule allows), and those workgroups take M from
 * their arguments instead of loading the header -- the same rows in the same tiles, results bit for bit the same; the
 * workgroup count spx_igemm_fwd_stats reports shrinks with the grid.  The contract: only for a blob whose header the
 * caller has read (never a prediction or an estimate: rows past a too-small M would not be computed), M exact, class
 * 1.  An M that does not fit the bits, or that exceeds n / 4, means no hint; without the hint, and for every other
 * dtype and for wider layers, the launch is what it is without the bits.  spx_launch_count("sparse_hint/v4") and
 * ("sparse_hint/bwd") count the launches that were shaped by it. */
#define SPX_SPARSE_ROWS_HINT 0x200
#define SPX_SPARSE_ROWS_SHIFT 12
#define SPX_SPARSE_ROWS_MAX 0x7ffff
#define SPX_ROWS_LAYOUT_ACT 0x400
/* OR-ed into `act` of spx_igemm_fwd_int8 next to SPX_ROWS_LAYOUT_ACT: the HOST knows the class word is 1 (it may
 * read it once per rulebook, outside any timed or captured region) -- a launch-shape hint only: 64-row instead
 * of 128-row tiles at 128 output channels (the role of the reference's per-problem tuner cache,
 * csrc/sparse/convops.py:1150,1283-1297).  Bits 16..31 of `act` may then carry ceil(M / 64), M = the blob's
 * word [1]: only that many appendix rows get workgroups (instead of the n / 4 the class rule allows).
 * Results never depend on either. */
#define SPX_SPARSE_HINT 0x800
#define SPX_LAYOUT_HEADER 64
size_t spx_subm_layout_bytes(int n, int kv);
size_t spx_subm_layout_ws_bytes(int n);
int spx_subm_layout(const int32_t *pair_fwd, const uint32_t *mask, int n, int kv, int32_t *layout,
                    void *ws, size_t ws_bytes, spx_stream_t stream);

/* Scratch for dgrad (always 0: the weight transpose happens inside the kernel). */
size_t spx_igemm_dgrad_ws_bytes(int C, int K, int kv, int dtype);

/* Input gradient.  Replaces the dgrad half of ConvGemmOps.implicit_gemm_backward
 * (convops.py:2245-2440, ops.py:1667-1896):
 *   din[i,:] = sum_k [pair_bwd[k][i] >= 0] dout[pair_bwd[k][i],:] * W[:,k,:]
 * For SubM pass subm=1 with the FORWARD pair/mask (mirror symmetry
 * pair_bwd[k] == pair_fwd[kv-1-k]; the reference's reverse_mask, convops.py:2327-2345).
 * dtype: SPX_F32 / SPX_F16 / SPX_BF16 / SPX_F64, as spx_igemm_fwd. */
int spx_igemm_dgrad(const void *dout, const void *weight, void *din, const int32_t *pair,
                    const uint32_t *mask, const int32_t *argsort, int tile_order, int n_out, int n_in,
                    int C, int K, int kv, int dtype, int subm, void *ws, size_t ws_bytes,
                    spx_stream_t stream);

/* Scratch for wgrad (per-workgroup fp32 partials + room for a work plan). */
size_t spx_igemm_wgrad_ws_bytes(int n_in, int C, int K, int kv);
/* The same for a given dtype: SPX_F64 needs float64 partial tiles (one per offset, fixed chunk of its pair list and
 * 64 x 64 tile of dW), which the query above cannot express; the other dtypes return spx_igemm_wgrad_ws_bytes.  Also
 * the scratch of spx_igemm_bwd. */
size_t spx_igemm_wgrad_ws_bytes_dtype(int n_in, int C, int K, int kv, int dtype);

/* Work plan of wgrad: the list of (offset, chunk-of-pairs) items that exist for a
 * rulebook, so the wgrad grid holds no empty workgroups.  It depends only on
 * num_per_loc, so callers build it once per rulebook and pass it to every
 * spx_igemm_wgrad call (plan == NULL makes wgrad rebuild it in `ws`). */
size_t spx_wgrad_plan_bytes(int n_in, int kv);
int spx_wgrad_plan(const int32_t *num_per_loc, int n_in, int kv, int subm, int32_t *plan,
                   spx_stream_t stream);

/* Weight gradient.  Replaces the wgrad half of implicit_gemm_backward and of
 * ConvGemmOps.indice_conv_backward (convops.py:1749-1860):
 *   dW[:,k,:] = sum_j dout[pair_native[1][k][j],:]^T (x) feat[pair_native[0][k][j],:]
 * over the Native lists; deterministic two-stage reduction (no atomics).
 *   dw KRSC [K, kv, C] in `dtype`, fully overwritten.
 *   subm=1: centre offset is the identity over all rows and offsets k > kv/2 use
 *   num_per_loc[kv-1-k] (ops.py:962-968).
 *   dtype SPX_F64: float64 partial tiles over fixed chunks of each list, summed in chunk order by a second launch (no
 *   atomics, bit-identical between calls); any kv; `plan` is not read; ws as spx_igemm_wgrad_ws_bytes_dtype. */
int spx_igemm_wgrad(const void *feat, const void *dout, void *dw, const int32_t *pair_native,
                    const int32_t *num_per_loc, const int32_t *plan, int n_in, int n_out, int C,
                    int K, int kv, int dtype, int subm, void *ws, size_t ws_bytes,
                    spx_stream_t stream);

/* Backward of a NARROW layer (C, K in {16, 32}, 16-bit features, kernel volume <= 27) from one gather per pair
 * (csrc/igemm_bwdn.hip): a walk over 128-row tiles of the input rows feeds every gathered dout tile to the
 * input gradient AND to the weight gradient.  Same role as spx_igemm_bwd (ConvGemmOps.implicit_gemm_backward,
 * pytorch/ops.py:1667-1896), without the Native lists and the range plan:
 *   table [kv, n_in], mask [n_in]: the dgrad table (SubM: pair_fwd; regular conv: pair_bwd) and its mask words
 *   weight_t [kv, C, K]: the weights with the dout channel contiguous, weight_t[k][c][k'] = weight[k'][k][c];
 *                        mirror = 1 (SubM): table row r pairs with slice kv-1-r
 *   din [n_in, C] or NULL;  dw KRSC [K, kv, C] in `dtype`, fully overwritten (deterministic)
 *   ws: spx_igemm_bwd_rows_ws_bytes (per-workgroup fp32 partial weight gradients) */
size_t spx_igemm_bwd_rows_ws_bytes(int n_in, int C, int K, int kv);
int spx_igemm_bwd_rows(const void *feat, const void *dout, const void *weight_t, void *din, void *dw,
                       const int32_t *table, const uint32_t *mask, int n_in, int n_out, int C, int K,
                       int kv, int mirror, int dtype, void *ws, size_t ws_bytes, spx_stream_t stream);

/* Backward of one layer: din (as spx_igemm_dgrad) and dw (as spx_igemm_wgrad) from ONE kernel
 * launch plus the wgrad second stage.  Replaces ConvGemmOps.implicit_gemm_backward /
 * indice_conv_backward as a whole (pytorch/ops.py:1667-1896,1103-1447), which also return both
 * gradients from one call.  pair / mask / argsort are the dgrad table (the FORWARD table for
 * SubM), pair_native / num_per_loc / plan as for spx_igemm_wgrad, ws as spx_igemm_wgrad_ws_bytes.
 * Shapes the fused kernel does not cover fall back to the two separate calls internally; so does SPX_F64 (ws as
 * spx_igemm_wgrad_ws_bytes_dtype). */
int spx_igemm_bwd(const void *feat, const void *dout, const void *weight, void *din, void *dw,
                  const int32_t *pair, const uint32_t *mask, const int32_t *argsort, int tile_order,
                  const int32_t *pair_native, const int32_t *num_per_loc, const int32_t *plan,
                  int n_in, int n_out, int C, int K, int kv, int dtype, int subm, void *ws,
                  size_t ws_bytes, spx_stream_t stream);

/* The weight gradient's SECOND STAGE deferred.  spx_igemm_bwd / spx_igemm_wgrad end with a small launch that reduces
 * the per-range partial tiles (fp32, in `ws`) into dw; nothing in a backward pass waits for a layer's dw, and a
 * dependent 4-9 us launch per layer is what a captured training step of a backbone is made of.  The *_deferred forms
 * run everything BUT that launch and write its description into `stage2_job` (SPX_STAGE2_JOB_BYTES bytes of host
 * memory, opaque); spx_wgrad_stage2_batch then reduces the partial tiles of up to 16 layers per launch (jobs:
 * `njobs` consecutive records, any mix of dtypes).  Between the two calls the caller keeps `ws`, the plan and dw
 * alive and must not read dw.  A call whose shapes take a path without a second stage (empty scene, odd channel counts)
 * completes dw at once and leaves an empty record, which the batch call skips.  Results are bit-identical to the
 * undeferred calls (same kernel body, same summation order).  The reference returns din and dw from one blocking
 * call (pytorch/ops.py:1667-1896); its split-K reduction is part of that call.  SPX_F64 is rejected (no deferred stage:
 * use spx_igemm_bwd / spx_igemm_wgrad). */
#define SPX_STAGE2_JOB_BYTES 64
int spx_igemm_bwd_deferred(const void *feat, const void *dout, const void *weight, void *din, void *dw,
                           const int32_t *pair, const uint32_t *mask, const int32_t *argsort, int tile_order,
                           const int32_t *pair_native, const int32_t *num_per_loc, const int32_t *plan,
                           int n_in, int n_out, int C, int K, int kv, int dtype, int subm, void *ws,
                           size_t ws_bytes, spx_stream_t stream, void *stage2_job);
int spx_igemm_wgrad_deferred(const void *feat, const void *dout, void *dw, const int32_t *pair_native,
                             const int32_t *num_per_loc, const int32_t *plan, int n_in, int n_out, int C,
                             int K, int kv, int dtype, int subm, void *ws, size_t ws_bytes,
                             spx_stream_t stream, void *stage2_job);
int spx_wgrad_stage2_batch(const void *jobs, int njobs, spx_stream_t stream);
/* Points a pending record at another destination of the same shape and dtype (an autograd engine may have moved the
 * gradient it was handed into a tensor of its own); returns 1, or 0 for an empty record. */
int spx_stage2_job_retarget(void *stage2_job, void *dw);

/* In-place epilogues for callers that keep bias/activation separate
 * (InferenceOps.bias_add_act_inplace etc., csrc/sparse/inference.py:26-146).  dtype: SPX_F32 / F16 / BF16 / F64. */
int spx_bias_act_inplace(void *out, const void *bias, int n, int K, int dtype, int act,
                         float act_alpha, spx_stream_t stream);

/* ------------------------------------------------------------------ pooling */

/* Sparse max / average pooling over the same rulebook tables.
 * Replace IndiceMaxPool::forward_implicit_gemm / backward_implicit_gemm /
 * forward_avgpool_implicit_gemm / backward_avgpool_implicit_gemm
 * (csrc/sparse/maxpool.py:96-300,397-588; pytorch/ops.py:1899-2084).
 *   pair_fwd [kv, n_out] / pair_bwd [kv, n_in] with -1 = absent; mask (one uint32 word per 32
 *   offsets and row) is optional and only used to skip absent offsets.
 *   max forward: out[o] = max over the valid pairs; init_zero != 0 starts from 0 instead of the
 *   lowest value (the reference's ConvAlgo.Native pooling does, pytorch/ops.py:1910).
 *   max backward: din[i] = sum of dout[o] over the outputs o with out[o] == feat[i].
 *   avg forward: mean over the valid pairs, count_out [n_out] (or NULL) receives their number.
 *   avg backward: din[i] = sum_o dout[o] / count[o].
 * dtypes: f32 / f16 / bf16 / f64 (float64 sums), plus int8 for the max forward. */
int spx_maxpool_fwd(const void *feat, void *out, const int32_t *pair_fwd, const uint32_t *mask,
                    int n_out, int C, int kv, int dtype, int init_zero, spx_stream_t stream);
int spx_maxpool_bwd(const void *feat, const void *out, const void *dout, void *din,
                    const int32_t *pair_bwd, const uint32_t *mask_bwd, int n_in, int C, int kv,
                    int dtype, spx_stream_t stream);
int spx_avgpool_fwd(const void *feat, void *out, int32_t *count_out, const int32_t *pair_fwd,
                    const uint32_t *mask, int n_out, int C, int kv, int dtype,
                    spx_stream_t stream);
int spx_avgpool_bwd(const void *dout, void *din, const int32_t *count, const int32_t *pair_bwd,
                    const uint32_t *mask_bwd, int n_in, int C, int kv, int dtype,
                    spx_stream_t stream);

/* ------------------------------------------------------------ point -> voxel */

/* Voxeliser.  Replaces SpconvOps.point2voxel_cuda / point2voxel_cpu
 * (csrc/sparse/all.py:1389-1500, csrc/sparse/pointops.py; driver pytorch/utils.py:23-160).
 * Result identical to the reference's CPU loop: voxels numbered in first-seen point order, the
 * first max_points points of a voxel kept in point order, voxels beyond max_voxels dropped.
 *   points [n, nfeat] fp32, the first ndim columns are x, y, z(, t)
 *   vsize [ndim], coors_range [2 ndim] (lows, then highs), grid_size [ndim]: all in ZYX order as
 *   returned by calc_point2voxel_meta_data (all.py:1349-1386)
 *   voxels [max_voxels, max_points, nfeat] fp32, indices [max_voxels, ndim] (zyx),
 *   num_per_voxel [max_voxels], pc_voxel_id [n] int64 (-1 = dropped point)
 *   empty_mean: 1 = unused slots of a voxel receive the mean of its points; 2 = the fill as the reference's CPU
 *   loop BEHAVES (pointops.py:663-686: its accumulator is carried from voxel to voxel), bit-identical to that
 *   code executed, a sequential pass (SPCONV_AMD_REFERENCE_QUIRKS=1 selects it in the Python layer);
 *   clear_voxels: zero `voxels` first.  *n_voxels_h receives the number of voxels (one D->H read). */
size_t spx_point2voxel_ws_bytes(int n_points, int max_voxels);
int spx_point2voxel(const float *points, int n, int nfeat, int ndim, const float *vsize,
                    const float *coors_range, const int *grid_size, int max_voxels, int max_points,
                    int empty_mean, int clear_voxels, float *voxels, int32_t *indices,
                    int32_t *num_per_voxel, long long *pc_voxel_id, int *n_voxels_h, void *ws,
                    size_t ws_bytes, spx_stream_t stream);

/* The voxeliser with static shapes: nothing is read back -- no copy to the host, no stream synchronisation, every
 * grid a function of host-known sizes, one stream -- so the call can be recorded in a stream capture in front of a
 * captured backbone pass (spconv_amd/pytorch/static.py).
 *   points [n_cap, nfeat] fp32; *n_points_dev (device int32): only rows below it are points, the rows behind it may
 *   hold anything (NaN included), get pc_voxel_id -1 and touch nothing else
 *   point_batch [n_cap] device int32 or NULL (every point in scene 0): the batch index is the leading digit of the
 *   voxel key; a point whose batch index is outside [0, batch_size) is dropped like a point outside the range
 *   vsize / coors_range / grid_size: host arrays in ZYX order, as spx_point2voxel
 *   indices [max_voxels, ndim + 1]: batch index, then zyx (the layout of a SparseConvTensor)
 *   num_per_voxel [max_voxels], pc_voxel_id [n_cap] int64
 *   voxels [max_voxels, max_points, nfeat] fp32, or NULL (only the mean is wanted): neither cleared nor written
 *   n_voxels_dev (device int32 [2]) = {voxels kept, voxels found}; found > kept: the scene hit max_voxels
 *   DEAD ROWS: every row >= kept comes out dead on every call, whatever the call before left there: -1 in every
 *   column of indices, count 0, zeros in voxels and mean_out (the padding contract of the static runners).
 * key_order = 0: voxels numbered first-seen by point index over the whole array, the first max_points points of a
 *   voxel kept in point order, voxels past max_voxels dropped.  With batch_size 1 and point_batch NULL the live rows
 *   of the zyx columns, of num_per_voxel, voxels and pc_voxel_id equal spx_point2voxel's bit for bit.  Grids beyond
 *   2^32 cells take the 64-bit-key form of the hash table.
 * key_order = 1: the same kept set (at the cap: the first max_voxels voxels in first-seen order), numbered by
 *   ascending linear key (batch-major, last axis fastest); pc_voxel_id, the stored points and the counts follow.
 *   With rankmap (>= spx_rankmap_bytes(ndim, batch_size, grid_size) bytes) the call leaves the level's rank map of
 *   `indices` behind: every key answers with its row, as in the map spx_rankmap_from_sorted builds from the same
 *   rows; keys are unique by construction, there is no violation flag.  Needs batch x grid <= 0xffe00000 cells and a
 *   rank map of at most 1 GiB: beyond that the call (and the workspace query: 0) fails -- number first-seen and sort.
 * mean_out [max_voxels, nfeat] of mean_dtype SPX_F32 / SPX_F16 / SPX_BF16, or NULL: row v = the stored points
 *   j = 0 .. num - 1 of voxel v added in that order in fp32, divided by num in fp32, rounded to nearest-even; computed
 *   from the points, never from the empty-slot fill.
 * empty_mean: 0 or 1 (1 needs voxels); 2, the sequential reference-quirk recurrence, stays with spx_point2voxel.
 * ws >= spx_point2voxel_static_ws_bytes(...) bytes (key_order = 1: + a rank map of the call's own for a caller that
 * passes none). */
size_t spx_point2voxel_static_ws_bytes(int n_cap, int max_voxels, int ndim, int batch_size, const int *grid_size,
                                       int key_order);
int spx_point2voxel_static(const float *points, const int32_t *point_batch, int n_cap, const int32_t *n_points_dev,
                           int nfeat, int ndim, const float *vsize, const float *coors_range, const int *grid_size,
                           int batch_size, int max_voxels, int max_points, int empty_mean, int key_order,
                           float *voxels, int32_t *indices, int32_t *num_per_voxel, long long *pc_voxel_id,
                           int32_t *n_voxels_dev, void *mean_out, int mean_dtype, void *rankmap, size_t rankmap_bytes,
                           void *ws, size_t ws_bytes, spx_stream_t stream);

/* ---------------------------------------------------------------- hash table */

/* Fixed-size hash table over caller-owned storage.  Replaces
 * spconv/csrc/hash/core.py HashTable as driven by spconv/pytorch/hash.py:29-170.
 *   table_keys [capacity] (4- or 8-byte integers, all-ones = empty; initialise with
 *   spx_hash_clear), table_vals [capacity] (4- or 8-byte items, copied bit for bit).  Linear probing from the home slot
 *   of a key; a slot, once taken, is never emptied.
 * The contract:
 *   - The all-ones key marks an empty slot and is never a member: insert ignores it (no slot claimed, no value written),
 *     query and insert_exist report it absent (is_empty = 1, nothing copied).
 *   - insert: values may be NULL (key only: table_vals is not written).  A key that finds no free slot is dropped and
 *     later reported absent: a table never holds more than `capacity` keys and never holds one twice.  Copies of one
 *     key within one call take one slot, and its value is one of the values given for that key.
 *   - query: is_empty[i] = 1 where the key is absent, 0 where it is present; values_out[i] is written only where the key
 *     is present -- the rows of absent keys keep the caller's bytes.
 *   - insert_exist: writes values only where the key is already present; is_empty as for query.
 *   - assign_arange: every present key gets as value its rank among the occupied slots in ascending SLOT index; items:
 *     the entries in the same order.  Two calls on an unchanged table agree bit for bit.  Which of two colliding keys
 *     holds the earlier slot is decided by the order the inserts arrive in, so the numbering depends on the slot
 *     contents, hence on insertion and arrival order -- not on the key set alone.
 *   - *count_out (may be NULL) is an integer of the KEY width and receives the number of keys, also when max_out is
 *     smaller; items writes nothing at or beyond min(count, max_out).
 *   - Refused before any device work: key_bytes / val_bytes other than 4 or 8, NULL table storage, capacity <= 0, n < 0,
 *     keys = NULL with n > 0, values_out = NULL (query) or values = NULL (insert_exist) with n > 0, max_out < 0,
 *     keys_out or vals_out = NULL with max_out > 0, ws = NULL or ws_bytes < spx_hash_ws_bytes(capacity) for
 *     assign_arange / items (ws need not be initialised).  n = 0 is a valid call that does nothing. */
size_t spx_hash_ws_bytes(int capacity);
int spx_hash_clear(void *table_keys, int capacity, int key_bytes, spx_stream_t stream);
int spx_hash_insert(void *table_keys, void *table_vals, int capacity, int key_bytes, int val_bytes,
                    const void *keys, const void *values, int n, spx_stream_t stream);
int spx_hash_query(void *table_keys, void *table_vals, int capacity, int key_bytes, int val_bytes,
                   const void *keys, void *values_out, unsigned char *is_empty, int n,
                   spx_stream_t stream);
int spx_hash_insert_exist(void *table_keys, void *table_vals, int capacity, int key_bytes,
                          int val_bytes, const void *keys, const void *values,
                          unsigned char *is_empty, int n, spx_stream_t stream);
int spx_hash_assign_arange(void *table_keys, void *table_vals, int capacity, int key_bytes,
                           int val_bytes, void *count_out, void *ws, size_t ws_bytes,
                           spx_stream_t stream);
int spx_hash_items(void *table_keys, void *table_vals, int capacity, int key_bytes, int val_bytes,
                   void *keys_out, void *vals_out, int max_out, void *count_out, void *ws,
                   size_t ws_bytes, spx_stream_t stream);

/* ---- batch normalisation (+ ReLU) over the features of a sparse tensor ---------------------------
 * The reference hands `.features` of a SparseConvTensor to torch.nn.BatchNorm1d (SparseSequential,
 * spconv/pytorch/modules.py:131-145; SparseBatchNorm / SparseReLU, :147-185).  These two calls do
 * the same arithmetic (torch.nn.BatchNorm1d semantics: biased variance to normalise, unbiased for
 * the running estimate, `momentum`, `eps`, optional affine) as three streaming launches per pass.
 *   x, y, dy, dx      [n, C] row-major, dtype f16 / bf16 / f32, C a multiple of 8 (f32: 4), C <= 65536.
 *                     Beyond 256 channels the row-streaming launches run over column blocks of 256 channels
 *                     (the last may be narrower); each channel is summed in the order the 256-wide kernel
 *                     sums it on a contiguous copy of its column block, so the results agree bit for bit
 *   weight, bias      [C] or NULL;  running_mean / running_var [C] or NULL (updated in place when
 *                     training, read when not)
 *   save_mean / save_invstd [C] fp32: batch statistics for the backward pass (training)
 *   relu              fuse max(0, .) into the output (and its mask into the backward pass)
 *   ws                spx_batchnorm_ws_bytes(n, C) bytes
 *   n_live            NULL, or a DEVICE int32: only the first *n_live rows are rows of the scene (static-shape
 *                     tensors, see spx_conv_rulebook_static): statistics over those rows, the others come out
 *                     as zeros (y and dx) */
size_t spx_batchnorm_ws_bytes(int n, int C);
/* weight / bias / running_mean / running_var: [C] vectors of dtype `param_dtype` (SPX_F32, or the
 * 16-bit dtype of a model converted with .half() / .bfloat16()); any of them may be NULL.
 * num_batches_tracked: the module's int64 step counter (torch/nn/modules/batchnorm.py:160-175), incremented by
 * the statistics kernel in training mode, or NULL. */
int spx_batchnorm_fwd(const void *x, void *y, int n, int C, int dtype, const void *weight,
                      const void *bias, void *running_mean, void *running_var,
                      long long *num_batches_tracked, int param_dtype, int training, float momentum,
                      float eps, int relu, float *save_mean, float *save_invstd, void *ws,
                      size_t ws_bytes, const int32_t *n_live, spx_stream_t stream);
/* Training-mode forward whose statistics pass has already happened: `stats` = the {rows, mean, M2} records
 * (stats_records of them, laid out [3][C][stats_records] fp32) that spx_igemm_fwd_stats left behind the convolution producing x.  Two
 * launches (merge, apply) instead of three; semantics as spx_batchnorm_fwd with training = 1.
 * n = 0 with records given still runs the merge: running estimates, num_batches_tracked and save_mean / save_invstd
 * come out as on a caller with rows (a SyncBatchNorm rank without voxels); only the apply launch is skipped. */
int spx_batchnorm_fwd_stats(const void *x, void *y, int n, int C, int dtype, const void *weight,
                            const void *bias, void *running_mean, void *running_var,
                            long long *num_batches_tracked, int param_dtype, float momentum, float eps,
                            int relu, float *save_mean, float *save_invstd, const float *stats,
                            int stats_records, const int32_t *n_live, spx_stream_t stream);
/* use_batch_stats = 1: `mean` / `invstd` are the saved fp32 batch statistics (training);
 * 0: fp32 copies of running_mean and 1 / sqrt(running_var + eps) (evaluation mode with gradients).
 * dweight / dbias: [C] of `param_dtype`, or NULL. */
int spx_batchnorm_bwd(const void *x, const void *dy, void *dx, int n, int C, int dtype,
                      const void *weight, const void *bias, int param_dtype, const float *mean,
                      const float *invstd, int use_batch_stats, int relu, void *dweight, void *dbias,
                      void *ws, size_t ws_bytes, const int32_t *n_live, spx_stream_t stream);

/* ---- SyncBatchNorm: the launches above, cut where the ranks of a process group exchange statistics ------------
 * The library issues no collective; the caller does (spconv_amd/pytorch/norm.py: one all-gather forward, one
 * all-reduce backward).  Forward: spx_batchnorm_local_stats -> all-gather of the records -> spx_batchnorm_fwd_stats
 * with stats = [3][C][world], stats_records = world.  Backward: spx_batchnorm_bwd_sums -> all-reduce of `sums` ->
 * spx_batchnorm_bwd_apply.  Shapes, dtypes, parameter dtypes, n_live and column blocks as above.
 *
 * A record counts rows in fp32, which is exact up to 2^24: spx_batchnorm_local_stats refuses n > 2^24, and the caller
 * must keep the TOTAL over all ranks at or below 2^24 rows (the total exists only on the device; norm.py refuses
 * rows x world > 2^24 on the host before any collective).
 *
 * spx_batchnorm_local_stats: record_out [3][C] fp32 = {live rows, mean, M2 (sum of squared deviations)} per channel
 * of this caller's rows.  stats_in = NULL: one pass over x (ws: spx_batchnorm_ws_bytes(n, C)) and a merge.  Otherwise
 * stats_in = the [3][C][stats_in_records] records spx_igemm_fwd_stats left: the merge alone, x is never read (may be
 * NULL).  n = 0 or *n_live = 0: a record of zero rows, which every merge skips; not an error.  No running estimate
 * is touched. */
int spx_batchnorm_local_stats(const void *x, int n, int C, int dtype, const float *stats_in,
                              int stats_in_records, float *record_out, void *ws, size_t ws_bytes,
                              const int32_t *n_live, spx_stream_t stream);
/* The two reduction launches of spx_batchnorm_bwd (batch statistics): sums [2][C] fp32, caller-owned =
 * {sum dy, sum dy * xhat} over this caller's live rows (dy masked by the ReLU when relu = 1).  dweight / dbias
 * ([C] of param_dtype, or NULL) are written from these LOCAL sums: SyncBatchNorm's parameter gradients are local and
 * the gradient all-reduce of data-parallel training averages them.  n = 0 writes zeros. */
int spx_batchnorm_bwd_sums(const void *x, const void *dy, int n, int C, int dtype, const void *weight,
                           const void *bias, int param_dtype, const float *mean, const float *invstd,
                           int relu, float *sums, void *dweight, void *dbias, void *ws, size_t ws_bytes,
                           const int32_t *n_live, spx_stream_t stream);
/* The apply launch of spx_batchnorm_bwd with the sums of ALL ranks: dx = w * invstd * (dy - sums[0] / N - xhat *
 * sums[1] / N), N = *total_rows, a DEVICE fp32 scalar holding the live rows of all ranks (summed from the gathered
 * records on the device; 0 gives dx = w * invstd * dy').  ReLU mask and zeroed padding rows as spx_batchnorm_bwd. */
int spx_batchnorm_bwd_apply(const void *x, const void *dy, void *dx, int n, int C, int dtype,
                            const void *weight, const void *bias, int param_dtype, const float *mean,
                            const float *invstd, int relu, const float *sums, const float *total_rows,
                            const int32_t *n_live, spx_stream_t stream);

/* ---- sparse <-> dense conversion (csrc/dense.hip) ---------------------------------------------------
 * Replace the torch composites of the reference's spconv/pytorch/core.py: `scatter_nd` (:44-57, a zero fill and an
 * index_put), `SparseConvTensor.dense` (:309-320, scatter_nd + permute().contiguous()) and `from_dense` (:296-307,
 * Tensor.to_sparse).  The kernels move bytes: elem_bytes is 1, 2, 4 or 8, any dtype of that size.
 *
 * The CELL MAP: map [batch * prod(spatial)] int32, map[cell] = the row that owns the cell, -1 = none; cell = the
 * row-major index over (batch, *spatial).  batch * prod(spatial) must fit int32; spx_dense_ws_bytes() gives the
 * bytes of the map (0 for an empty grid, and for one that is too large).
 *   spx_dense_map: skips row r when its batch index is < 0 or >= batch, when a coordinate is outside
 *   [0, extent), and when r >= *n_live (n_live: NULL or a device int32, see spx_conv_rulebook_static).  Of
 *   several rows with the same coordinate the HIGHEST row number owns the cell, on every call.
 *   spx_to_dense: out = [batch, *spatial, C] (channels_first = 0) or [batch, C, *spatial] (1); every element is
 *   written exactly once: rows[map[cell]] or the fill value (fill_bits: bit pattern of one element in the low
 *   elem_bytes bytes; 0 = zero, a quantised tensor passes its zero point).  rows [n, C] with a row stride of
 *   row_stride elements (>= C).  A map entry outside [0, n) counts as -1 here and in spx_dense_gather: the map is
 *   the caller's memory, a stale one must not turn into an access outside `rows`.
 *   spx_dense_gather: the inverse, rows [n, C] contiguous: rows[map[cell]] = dense[cell]; a row that owns no
 *   cell (dead, out of range, or a duplicate that lost) receives zeros.  Backward of spx_to_dense. */
size_t spx_dense_ws_bytes(int ndim, int batch, const int *spatial_h);
int spx_dense_map(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch,
                  const int *spatial_h, int32_t *map, spx_stream_t stream);
int spx_to_dense(const void *rows, int n, long long row_stride, const int32_t *map, void *out, int C,
                 int elem_bytes, int channels_first, long long fill_bits, int ndim, int batch,
                 const int *spatial_h, spx_stream_t stream);
int spx_dense_gather(const void *dense, const int32_t *map, void *rows, int n, int C, int elem_bytes,
                     int channels_first, int ndim, int batch, const int *spatial_h,
                     spx_stream_t stream);
/* from_dense: dense = channels-last [batch, *spatial, C], contiguous.  A cell is active when any of its channels
 * compares unequal to zero (is_float: -0.0 is zero, NaN is not -- Tensor.to_sparse).
 *   count: flags and counts the active cells into ws (spx_from_dense_ws_bytes) and reads the count back into
 *   *n_active_h (one D->H read, the data-dependent shape; synchronises the stream).
 *   fill: with the SAME ws, writes indices [n_active, ndim + 1] (ascending cell order = the order of
 *   to_sparse(...).indices()), rows [n_active, C] and, unless NULL, the cell map of the result. */
size_t spx_from_dense_ws_bytes(int ndim, int batch, const int *spatial_h);
int spx_from_dense_count(const void *dense, int C, int elem_bytes, int is_float, int ndim, int batch,
                         const int *spatial_h, void *ws, size_t ws_bytes, int *n_active_h,
                         spx_stream_t stream);
int spx_from_dense_fill(const void *dense, int C, int elem_bytes, int ndim, int batch,
                        const int *spatial_h, const void *ws, size_t ws_bytes, int32_t *indices,
                        void *rows, int32_t *map, spx_stream_t stream);

/* What the row operators may be handed (spx_union_count / _fill / _static, spx_union_add_fwd / _bwd, spx_collapse_count /
 * _fill / _static, spx_collapse_fwd / _bwd, spx_point_groups, spx_row_score, spx_topk_flags, spx_select_count / _fill /
 * _static, spx_point_corners in both lookup forms, spx_interp_fwd / _bwd, spx_group_fwd / _bwd: the operators that sit
 * between the layers); tests/test_gpu_rowop_isolation.py holds them to it, the references to it tests/test_refrowops.py:
 *   (a) Dirty memory on entry.  Every output, workspace, counter record (n_out_dev, sel_dev) and rank map may hold any
 *       bytes on entry: every element the caller reads afterwards has been stored, no region of a workspace or map is
 *       read before it is written.  The two-call forms keep their rule -- ws and rankmap unchanged between count and
 *       fill -- and the dirt is there before the count.  Regions a section below calls unspecified (list from
 *       offsets[n_out] on) stay unspecified.
 *   (b) Rows that nothing names may hold anything, NaN and Inf included, and change no output bit: feature rows at or
 *       beyond *n_live; rows whose index row is dead (batch index or a coordinate out of range); rows dropped by a cap;
 *       dout rows of points or queries that are invalid or lie at or beyond *n_points / *n_queries; dout entries of slots
 *       with rows == -1; corner_w entries whose corner_rows entry is -1.  Output rows past the live count are what the
 *       sections below promise: zeros or -1.
 *   (c) Named rows.  Nothing non-finite is swallowed: an output element is NaN, +Inf or -Inf exactly where the sequential
 *       sum (or maximum) over the named rows is.  The payload of a COMPUTED NaN is not part of the contract; a NaN that is
 *       moved (a copy, a gather, the max) keeps its bits.  A finite f16 / bf16 group whose fp32 sum exceeds the type's
 *       range rounds to +-Inf: the one rounding at the end.
 *         max (spx_collapse_fwd, SPX_COLLAPSE_MAX): NaN propagates.  The output element is the FIRST NaN of the group in
 *         list order, bits unchanged; without a NaN the first of the largest values, -0.0 / +0.0 compared as equal.
 *         max backward: where out[r, c] is NaN every row of the group whose feat[i, c] is NaN receives dout[r, c], the
 *         others 0 ("ties all receive"; not torch's silent zero: the gradient does not vanish where the forward said NaN).
 *         spx_row_score: a row with a NaN element scores a POSITIVE NaN under both ops, so it sorts above +inf.
 *         spx_topk_flags: the key order over ALL bit patterns -- a positive NaN above +inf, a negative NaN below -inf,
 *         NaNs among themselves by payload.  Which rows a caller's own non-finite scores select follows from that order
 *         alone.
 *   (d) Spreading.  spx_interp_fwd / _bwd are IEEE as written: a LIVE corner (row >= 0) whose weight is exactly 0 and whose
 *       row holds Inf or NaN contributes 0 x Inf = NaN.  The weight of an absent corner is never multiplied.  (Parallel
 *       to (d) of the gather-GEMM section.)
 *   (e) Non-finite weights in corner_w at live corners, and non-finite scores handed to spx_topk_flags, are the caller's:
 *       the arithmetic is IEEE and the key order above holds, nothing more is promised. */

/* ---- misaligned add (csrc/union.hip) -----------------------------------------------------------------
 * Replace the torch composite behind the reference's spconv/pytorch/functional.py:439-545 (sparse_add_hash_based,
 * sparse_add) and tables.py AddTableMisaligned: T hash inserts + an arange whose count is read back, T queries, T
 * index_add_ (float atomics: non-deterministic from three operands on), T indexed index writes and a zero fill.
 *
 * UNION of T coordinate sets, 1 <= T <= SPX_UNION_MAX_OPERANDS.  The operands arrive as HOST arrays of length T:
 * indices_h[t] = device int32 [n_h[t], ndim + 1], n_live_h (or NULL) with n_live_h[t] = NULL or a device int32 (see
 * spx_conv_rulebook_static).  A row is DEAD -- contributes nothing -- when it lies at or beyond *n_live_h[t], when its
 * batch index is outside [0, batch) or a coordinate outside [0, extent).  The union is numbered through the level's
 * RANK MAP (sorted-order levels above; the caller's buffer of spx_rankmap_bytes): byte marks, the prefix pass, one
 * 8-byte load per row -- no hash table, no atomic on the path that numbers the rows.
 *   spx_union_ws_bytes: scratch of a build over n_total = sum n_h[t] rows; 0 when the key space does not fit (as
 *   spx_rankmap_bytes: keep the hash path), for an empty grid and for T outside its range.
 *   spx_union_count: marks, prefix pass, ownership pass, and the call's ONE D->H read (synchronises the stream):
 *   result_h [2 + T] = {union size, duplicate flag, live rows of operand 0 .. T-1}.  The duplicate flag is 1 when a
 *   coordinate occurs twice within one operand: the composite sums such rows, a src table cannot say that -- the
 *   caller falls back.
 *   spx_union_fill: with the SAME rankmap and ws, unchanged since the count, writes
 *     rows_h[t]  device int32 [n_h[t]]: the output row of each input row, -1 for a dead or dropped row
 *     src        device int32 [T][n_out]: the row of operand t that sits at that output row, or -1
 *     out_indices [n_out, ndim + 1] (base = -1 only; may be NULL otherwise)
 *   base = -1: rows in ascending linear key order (batch-major, last axis fastest: the numbering of the sorted-order
 *   levels); n_out = the union size (a smaller n_out keeps the first n_out keys) and the rank map left behind
 *   describes the result, so spx_subm_rulebook_ranked applies to it.
 *   base = b: operand b's own numbering -- n_out = n_h[b], rows_h[b] = identity on its live rows, src of its dead rows
 *   = -1, the result's indices ARE operand b's.  Legal only when the host has seen live rows of b == union size and the
 *   duplicate flag 0 (b holds every coordinate of the union exactly once).
 *   spx_union_static: the static-shape form, always in key order: room for n_out_cap rows, nothing read back
 *   (hipGraph-safe; five launches).  n_out_dev [3] (device) = {union size found -- may exceed the cap --, duplicate
 *   flag, live rows = min(found, cap)}; out_indices rows past the live count are -1 (as spx_conv_rulebook_static
 *   writes them), their src entries -1; outputs beyond the cap are dropped in key order (rows_h entry -1).
 * With duplicates present every call still finishes with every index in range: of the rows of one operand with one
 * coordinate the HIGHEST row owns the cell (as spx_dense_map), on every call.
 *
 * ROW MERGE.
 *   spx_union_add_fwd: out[r, :] = sum over the operands t with src[t][r] >= 0, in operand order, of
 *   feat_h[t][src[t][r], :] ([n_h[t], C] contiguous), accumulated in fp32 (fp64 for SPX_F64) and rounded once to
 *   `dtype` (SPX_F16 / SPX_BF16 / SPX_F32 / SPX_F64).  An absent operand is skipped, not added as zero: a row held by
 *   one operand keeps its bits (-0.0 stays -0.0); a row held by none, and every row >= *n_live (NULL or a device
 *   int32), is zero.  Every output element is written exactly once: no zero fill, no atomics, one launch for all
 *   operands.  Any C >= 1: rows whose byte size is a multiple of 16 (and 16-byte aligned pointers) move as 16-byte
 *   pieces per lane, other widths element by element.  A src entry outside [0, n_h[t]) counts as -1.
 *   spx_union_add_bwd: din_h[t][i, :] = dout[rows_h[t][i], :], zeros where the entry is outside [0, n_out): a
 *   byte-moving gather for elem_bytes 2, 4 or 8, one launch for all operands.
 * Dirty buffers, unnamed rows and NaN / Inf: "What the row operators may be handed" above. */
size_t spx_union_ws_bytes(int ndim, int batch, const int *spatial_h, int T, long long n_total);
int spx_union_count(const int32_t *const *indices_h, const int *n_h, const int32_t *const *n_live_h, int T,
                    int ndim, int batch, const int *spatial_h, void *rankmap, size_t rankmap_bytes, void *ws,
                    size_t ws_bytes, int *result_h, spx_stream_t stream);
int spx_union_fill(const int32_t *const *indices_h, const int *n_h, const int32_t *const *n_live_h, int T,
                   int ndim, int batch, const int *spatial_h, int n_out, int base, int32_t *out_indices,
                   int32_t *const *rows_h, int32_t *src, const void *rankmap, size_t rankmap_bytes,
                   const void *ws, size_t ws_bytes, spx_stream_t stream);
int spx_union_static(const int32_t *const *indices_h, const int *n_h, const int32_t *const *n_live_h, int T,
                     int ndim, int batch, const int *spatial_h, int n_out_cap, int32_t *out_indices,
                     int32_t *const *rows_h, int32_t *src, int32_t *n_out_dev, void *rankmap,
                     size_t rankmap_bytes, void *ws, size_t ws_bytes, spx_stream_t stream);
int spx_union_add_fwd(const void *const *feat_h, const int *n_h, int T, const int32_t *src, int n_out, int C,
                      int dtype, void *out, const int32_t *n_live, spx_stream_t stream);
int spx_union_add_bwd(const void *dout, int n_out, void *const *din_h, const int32_t *const *rows_h,
                      const int *n_h, int T, int C, int elem_bytes, spx_stream_t stream);

/* ---- axis collapse (csrc/collapse.hip) -----------------------------------------------------------------
 * Drops spatial axes of a sparse tensor and merges the rows that land on one cell of the PROJECTED grid: the height
 * compression of the fully sparse detectors ((batch, z, y, x) rows -> (batch, y, x) rows, a SubMConv2d / SparseConv2d
 * head behind).  Stands where a torch composite would: unique of the projected keys (a count read back), index_add_
 * (float atomics: not reproducible), rows in `unique` order without a rank map, no notion of dead rows.
 *
 * indices = device int32 [n, ndim + 1], n_live = NULL or a device int32 (see spx_conv_rulebook_static).  axes_mask: bit
 * d set = spatial axis d (0 = the first, z of a zyx tensor) is removed; at least one axis stays; 0 is legal and merges
 * duplicate coordinates.  A row is DEAD -- contributes nothing -- when it lies at or beyond *n_live, when its batch index
 * is outside [0, batch) or ANY coordinate, a removed one included, outside [0, extent).  Live rows are grouped by their
 * projected coordinate (batch index + the kept axes in their order); a coordinate that occurs twice is two rows of its
 * group.  OUTPUT ROWS are the groups in ascending linear key of the projected grid (batch-major, last kept axis
 * fastest: the numbering of the sorted-order levels), numbered through the projected level's RANK MAP (the caller's
 * buffer of spx_rankmap_bytes(kept axes); left behind, it describes the result, so spx_subm_rulebook_ranked applies):
 * byte marks, the prefix pass, one 8-byte load per row -- no hash table, no atomic on the path that numbers the rows.
 * THE ROWS OF A GROUP ARE LISTED IN ASCENDING INPUT ROW: the list is a stable radix argsort of the rows by their rank
 * (dead rows take a key behind every rank), so the order is a property of the sort, not of any scheduling.
 *   spx_collapse_ws_bytes: scratch of a build over n rows; 0 when the projected key space does not fit (the rule of
 *   spx_rankmap_bytes on the projected grid), for an empty grid (any extent < 1), when no axis is kept, and for a mask
 *   that names an axis >= ndim.
 *   spx_collapse_count: marks, prefix pass, and the call's ONE D->H read (synchronises the stream):
 *   result_h [2] = {n_out = cells found, live input rows}.
 *   spx_collapse_fill: with the SAME rankmap and ws, unchanged since the count, writes
 *     out_indices [n_out, kept + 1]
 *     rows        [n]: the output row of each input row, -1 for a dead or dropped row
 *     offsets     [n_out + 1]: group r is list[offsets[r] .. offsets[r + 1])
 *     list        [n]: the input rows group after group, ascending inside a group; entries from offsets[n_out] on are
 *                 unspecified
 *   (a smaller n_out keeps the first n_out keys).  Launches: a one-word fill, rank, the sort (three per radix pass of
 *   8 or 9 bits over ceil(log2(n_out + 1)) bits), boundaries.
 *   spx_collapse_static: the static-shape form: room for n_out_cap rows (offsets [n_out_cap + 1]), nothing read back
 *   (hipGraph-safe).  n_out_dev [3] (device) = {cells found -- may exceed the cap --, 0, live = min(found, cap)}; groups
 *   beyond the cap are dropped in key order (rows entry -1); out_indices rows past the live count are -1, offsets
 *   entries past it equal offsets[live].
 *
 * REDUCTION.  op: SPX_COLLAPSE_SUM / _MEAN / _MAX; dtype SPX_F16 / SPX_BF16 / SPX_F32 / SPX_F64; any C >= 1: rows whose
 * byte size is a multiple of 16 (and 16-byte aligned pointers) move as 16-byte pieces per lane, other widths element by
 * element.  The argument checks (mask, dtype, C, op) come before any pointer is looked at.
 *   spx_collapse_fwd: out [n_out, C] from feat [n, C].  An output row belongs to a group of lanes that covers its
 *   pieces (a power of two, at most a wave; wider rows take several passes) and walks its list entries in order.
 *     sum:  the accumulator (fp32; fp64 for SPX_F64) starts from the first row's value and adds the others one by one
 *           in list order; one rounding to `dtype`.  A group of one row is copied bit for bit (-0.0 stays -0.0).  No
 *           atomics, no zero fill, every output element written exactly once: identical run to run, and reproducible
 *           on the host with a sequential loop.
 *     mean: that sum divided by the group's row count in fp32 (fp64), rounded once.
 *     max:  the maximum of the stored values (the first of equals): a copy of an input element.  A NaN in the group
 *           propagates: the output is the group's first NaN in list order, bits unchanged ("What the row operators may
 *           be handed", (c)).
 *   Rows at or beyond *n_live_out (NULL or a device int32) are written as zeros.  A list entry outside [0, n) is
 *   skipped.
 *   spx_collapse_bwd (mean and max; the gradient of a sum is spx_union_add_bwd with one operand): with r = rows[i],
 *     mean: din[i] = dout[r] / (offsets[r + 1] - offsets[r]), divided in fp32 (fp64), rounded once (feat / out unused)
 *     max:  din[i, c] = dout[r, c] where feat[i, c] == out[r, c], or where both are NaN, else 0: ties all receive, as
 *           spx_maxpool_bwd, and a NaN output sends its gradient to every NaN of its group (offsets unused)
 *   zeros where rows[i] is outside [0, n_out).
 * Dirty buffers, unnamed rows and NaN / Inf: "What the row operators may be handed" above. */
size_t spx_collapse_ws_bytes(int ndim, int batch, const int *spatial_h, int axes_mask, long long n);
int spx_collapse_count(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch,
                       const int *spatial_h, int axes_mask, void *rankmap, size_t rankmap_bytes, void *ws,
                       size_t ws_bytes, int *result_h, spx_stream_t stream);
int spx_collapse_fill(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch,
                      const int *spatial_h, int axes_mask, int n_out, int32_t *out_indices, int32_t *rows,
                      int32_t *offsets, int32_t *list, const void *rankmap, size_t rankmap_bytes, void *ws,
                      size_t ws_bytes, spx_stream_t stream);
int spx_collapse_static(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch,
                        const int *spatial_h, int axes_mask, int n_out_cap, int32_t *out_indices, int32_t *rows,
                        int32_t *offsets, int32_t *list, int32_t *n_out_dev, void *rankmap, size_t rankmap_bytes,
                        void *ws, size_t ws_bytes, spx_stream_t stream);
int spx_collapse_fwd(const void *feat, int n, const int32_t *offsets, const int32_t *list, int n_out, int C,
                     int dtype, int op, void *out, const int32_t *n_live_out, spx_stream_t stream);
int spx_collapse_bwd(const void *feat, const void *out, const void *dout, const int32_t *rows,
                     const int32_t *offsets, int n, int n_out, int C, int dtype, int op, void *din,
                     spx_stream_t stream);

/* ---- point <-> voxel features (csrc/pointvoxel.hip) ------------------------------------------------------
 * The three operations of a learned voxel feature encoder (the DynamicVFE / DynamicPillarVFE of the fully sparse
 * detectors) between a voxeliser and the first sparse layer: the points of every voxel as GROUPS, voxel rows carried
 * back to their points, and the decorated input row of the per-point MLP.  They stand where torch_scatter composites
 * would: argsort + bincount + cumsum, index_select + where, index_add_ (float atomics: not reproducible).  The
 * reductions over the groups (sum, mean, max over ALL points of a voxel) are spx_collapse_fwd / _bwd with the rows,
 * offsets and list made here; the gradient of spx_voxel_to_point is spx_collapse_fwd(dout, op = SPX_COLLAPSE_SUM) over
 * the same groups -- added in ascending point index in fp32 (fp64 for SPX_F64), rounded once, identical run to run.
 * Every call: the caller allocates, nothing is read back, nothing synchronises, every grid depends on host-known sizes
 * only (hipGraph-safe).  The argument checks that need no pointer come before any pointer is looked at.
 *
 *   spx_point_groups: ids = device [n_cap], int64 (id_bytes 8: the pc_voxel_id of spx_point2voxel / _static) or int32
 *   (id_bytes 4).  n_points_dev = NULL or a device int32: rows at or beyond it are no points, whatever they hold.  A
 *   point belongs to voxel v = ids[i] when 0 <= v < num_voxels (num_voxels >= 1); every other point, negative ids
 *   included, belongs to no voxel.  Outputs (device int32):
 *     rows    [n_cap]: v, or -1
 *     offsets [num_voxels + 1]: group v is list[offsets[v] .. offsets[v + 1]); an empty voxel is an empty range
 *     list    [n_cap]: the points group after group IN ASCENDING POINT INDEX; entries from offsets[num_voxels] on are
 *             unspecified
 *   The list is a stable radix argsort of the points by voxel id (the LSD radix of rowsort.hip over
 *   ceil(log2(num_voxels + 1)) bits; a point without a voxel takes the key num_voxels, behind every id), so the order
 *   inside a group is a property of the sort, not of any scheduling; offsets[v] is the first sorted position whose key
 *   is >= v (a bisection per voxel: runs of empty voxels cost nothing extra).  n_cap = 0 is legal (offsets all 0).
 *   Launches: the key pass, three per radix pass of 8 or 9 bits, the boundary pass.
 *   spx_point_groups_ws_bytes: its scratch; 0 for n_cap < 0 or num_voxels < 1.  Monotone in both arguments.
 *   Dirty buffers on entry: "What the row operators may be handed" (before the misaligned add), (a).
 *
 *   spx_voxel_to_point: out[i, :] = vfeat[rows[i], :] ([num_voxels, C] -> [n_cap, C], contiguous), or C copies of the
 *   fill element (the low elem_bytes bytes of fill_bits) where rows[i] is outside [0, num_voxels).  A byte-moving
 *   gather: elem_bytes 1, 2, 4 or 8, any C >= 1; rows whose byte size is a multiple of 16 (and 16-byte aligned
 *   pointers) move as 16-byte pieces per lane, other widths element by element.  One launch, no temporaries, every
 *   output element written exactly once.
 *
 *   spx_point_decorate: the input row of a dynamic VFE.  points = fp32 [n_cap, nfeat], the first ndim columns x, y, z
 *   (as spx_point2voxel); rows = spx_point_groups' (entries >= 0 are trusted to be voxel rows of `indices` and
 *   `cluster_mean`); indices = the voxel index rows [*, ndim + 1] (batch index, then zyx); vsize [ndim] and
 *   coors_range [2 * ndim] = HOST arrays in zyx order, as spx_point2voxel takes them; cluster_mean = fp32
 *   [num_voxels, nfeat] (spx_collapse_fwd(points, op = SPX_COLLAPSE_MEAN) over the groups; may be NULL without flag
 *   bit 0).  Row i of out [n_cap, C_out], with r = rows[i] and j = 0 .. ndim - 1 the columns x, y, z:
 *     the point's nfeat columns;
 *     flags & 1: points[i, j] - cluster_mean[r, j];
 *     flags & 2: points[i, j] - centre_j, centre_j = (float(c_j) + 0.5f) * vsize_j + lo_j with c_j the voxel's
 *                coordinate along that axis (indices[r, ndim - j]);
 *     zeros up to C_out (C_out >= nfeat + ndim * popcount(flags & 3)).
 *   A point without a voxel (r < 0) gets a row of zeros.  All arithmetic is fp32, every multiply, add and subtract
 *   rounded on its own (no contraction into an FMA: float32 arithmetic on the host reproduces every element bit for
 *   bit), then one round-to-nearest-even into out_dtype (SPX_F32 / SPX_F16 / SPX_BF16).  One launch. */
size_t spx_point_groups_ws_bytes(int n_cap, int num_voxels);
int spx_point_groups(const void *ids, int id_bytes, int n_cap, const int32_t *n_points_dev, int num_voxels,
                     int32_t *rows, int32_t *offsets, int32_t *list, void *ws, size_t ws_bytes,
                     spx_stream_t stream);
int spx_voxel_to_point(const void *vfeat, int num_voxels, const int32_t *rows, int n_cap, int C, int elem_bytes,
                       long long fill_bits, void *out, spx_stream_t stream);
int spx_point_decorate(const float *points, int nfeat, int n_cap, const int32_t *rows, const int32_t *indices,
                       int ndim, const float *vsize, const float *coors_range, const float *cluster_mean,
                       int flags, void *out, int out_dtype, int C_out, spx_stream_t stream);

/* ---- trilinear devoxelisation (csrc/interp.hip) ------------------------------------------------------------
 * Voxel rows of a sparse level interpolated to points: every point reads the K = 2^ndim voxels whose CENTRES surround
 * it and blends their rows (the devoxelize of SPVCNN / PVCNN, the point refinement of Cylinder3D, the voxel-to-keypoint
 * interpolation of the PV-RCNN family).  Stands where a torch composite would: K hash queries per point, index_select
 * + mul + sum over [N, K, C] temporaries, an index_add_ backward (float atomics: not reproducible), none of it aware of
 * dead rows or a device-side point count.  Every call: the caller allocates, nothing is read back, nothing
 * synchronises, every grid depends on host-known sizes only (hipGraph-safe).  The argument checks that need no pointer
 * come before any pointer is looked at.  There is no gradient with respect to the points or the weights.
 *
 *   spx_point_corners: points = fp32 [n_cap, nfeat], the first ndim columns x, y, z (as spx_point2voxel); batch_ids =
 *   int32 [n_cap] or NULL (all batch 0); n_points_dev = NULL or a device int32: rows at or beyond it are no points;
 *   ndim = 2 or 3, K = 2^ndim; vsize [ndim] and coors_range [2 * ndim] = HOST arrays in zyx order, as
 *   spx_point_decorate takes them -- the voxel size is that of the level being read; indices = int32 [n, ndim + 1], the
 *   level's index rows; n_live = NULL or a device int32; batch, spatial_h [ndim] = batch count and grid extents;
 *   rankmap = NULL or a buffer of spx_rankmap_bytes(ndim, batch, spatial_h); flags bit 0 = normalise.
 *   Outputs (device, 16-byte aligned): corner_rows int32 [n_cap, K], corner_w fp32 [n_cap, K].
 *   Per point column j (x = 0; grid axis ndim - 1 - j), all in fp32:
 *     t_j = (p_j - lo_j) / vsize_j          (the voxeliser's expression: the point's own voxel is floorf(t_j))
 *     g_j = t_j - 0.5f, b_j = floorf(g_j), f_j = g_j - b_j
 *   Corner c steps by bit j of c along axis j: coordinate b_j + bit, weight ((w_x * w_y) * w_z) with
 *   w_j = bit ? f_j : 1.0f - f_j.  A point is VALID when it lies below *n_points, its batch id is in [0, batch) and
 *   floorf(t_j) is in [0, extent_j) on every axis (false for NaN); an invalid point gets rows -1 and weights 0.  A
 *   corner outside the grid, or one that no LIVE row holds, gets row -1 and weight 0; a row is live when it lies below
 *   *n_live, its batch index is in [0, batch) and its coordinates are in range.  Normalise: s = the sum of the present
 *   corners' weights added in ascending corner index, every present weight becomes w / s, s == 0 leaves rows -1 and
 *   weights 0.  Every multiply, add, subtract and divide is rounded on its own (no FMA).
 *   Lookup: with a rank map the caller vouches that the live rows are in ascending, unique key order and the row is
 *   the rank of the key (one launch, no hash table, ws may be NULL).  With rankmap = NULL the call builds the hash
 *   table of the index builders in ws from the live rows' keys -- a duplicate coordinate goes to the lowest row -- and
 *   probes it: a fill, the insert pass, the corner pass.  Both forms return identical tables for a key-ordered,
 *   duplicate-free level.  Requires n_cap * K < 2^31.
 *   At most 2^30 rows (the table holds two slots per row), and batch x grid must fit a 63-bit key.
 *   spx_point_corners_ws_bytes: scratch of the hash form; monotone in its arguments, 0 for arguments that are refused
 *   (ndim outside {2, 3}, a negative count, n_cap * K >= 2^31, n > 2^30).
 *
 *   spx_interp_fwd: out[i, :] = sum over c = 0 .. K - 1 of corner_w[i, c] * vfeat[corner_rows[i, c], :] ([n, C] ->
 *   [n_cap, C], contiguous; SPX_F16 / SPX_BF16 / SPX_F32 / SPX_F64).  Corners whose row is outside [0, n) are skipped;
 *   fp32 accumulation (fp64 for SPX_F64) from zero in ascending c as acc = acc + (w * x), each operation rounded on its
 *   own, one round-to-nearest-even into the feature type; a point without a corner gets zeros.  Rows whose byte size is
 *   a multiple of 16 (and 16-byte aligned pointers) move as 16-byte pieces per lane, other widths element by element.
 *   One launch, no temporaries, every output element written exactly once.
 *
 *   spx_interp_bwd: the gradient with respect to the voxel rows over the TRANSPOSED corner list: offsets [n + 1] and
 *   list [n_cap * K] = spx_point_groups(ids = corner_rows flattened, id_bytes 4, n_cap * K entries, num_voxels = n),
 *   whose groups hold the entries e = i * K + c in ascending e.  dvfeat[v, :] = sum over e in list[offsets[v] ..
 *   offsets[v + 1]) of corner_w[e] * dout[e / K, :], in list order, accumulated and rounded as the forward; zeros for
 *   an empty group and for rows at or beyond *n_live.  No atomics, identical run to run; a voxel's row belongs to a
 *   group of lanes (the walk of spx_collapse_fwd), so long groups do not serialise on one lane.  One launch.
 * Dirty buffers, unnamed rows, NaN / Inf and the zero-weight live corner (0 x Inf = NaN spreads): "What the row operators
 * may be handed" (before the misaligned add), (a) - (e). */
size_t spx_point_corners_ws_bytes(int n_cap, int ndim, int n);
int spx_point_corners(const float *points, int nfeat, const int32_t *batch_ids, int n_cap,
                      const int32_t *n_points_dev, int ndim, const float *vsize, const float *coors_range,
                      const int32_t *indices, int n, const int32_t *n_live, int batch, const int *spatial_h,
                      const void *rankmap, size_t rankmap_bytes, int flags, int32_t *corner_rows, float *corner_w,
                      void *ws, size_t ws_bytes, spx_stream_t stream);
int spx_interp_fwd(const void *vfeat, int n, const int32_t *corner_rows, const float *corner_w, int n_cap, int ndim,
                   int C, int dtype, void *out, spx_stream_t stream);
int spx_interp_bwd(const void *dout, int n_cap, int ndim, const float *corner_w, const int32_t *offsets,
                   const int32_t *list, int n, const int32_t *n_live, int C, int dtype, void *dvfeat,
                   spx_stream_t stream);

/* ---- voxel query and neighbour grouping (csrc/query.hip) ---------------------------------------------------
 * Per query point the first `nsample` voxels of a sparse level inside a window of cells, optionally inside a radius,
 * and their rows gathered: the voxel_query / grouping_operation pair of the two-stage detectors over sparse backbones
 * (Voxel R-CNN's Voxel RoI pooling, the voxel set abstraction of the PV-RCNN family).  Stands where a torch composite
 * would: one hash query per window cell, a topk per query, index_select, an index_add_ backward (float atomics: not
 * reproducible).  Every call: the caller allocates, nothing is read back, nothing synchronises, every grid depends on
 * host-known sizes only (hipGraph-safe).  The argument checks that need no pointer come before any pointer is looked
 * at.  There is no gradient with respect to the queries.
 *
 *   spx_voxel_query: queries = fp32 [n_cap, nfeat], the first ndim columns x, y, z; batch_ids = int32 [n_cap] or NULL
 *   (all batch 0); n_queries_dev = NULL or a device int32: rows at or beyond it are no queries; ndim = 2 or 3; vsize
 *   [ndim], coors_range [2 * ndim], indices, n, n_live, batch, spatial_h, rankmap: as spx_point_corners takes them;
 *   query_range [ndim] = HOST ints in index-column (zyx) order, each in 0 .. 15; nsample in 1 .. 128; r2 = the squared
 *   radius, computed by the caller in fp32; flags = 1 (apply the radius test) | 2 (pad = first) | w << 8 (w = 0: the
 *   group width is chosen from the window; w = 1 .. 7: 2^(w - 1) lanes per query -- the result is the same).
 *   Outputs (device): rows int32 [n_cap, nsample], count int32 [n_cap], offsets fp32 [n_cap, nsample, ndim] or NULL.
 *   Per point column j (x = 0; grid axis ndim - 1 - j): t_j = (q_j - lo_j) / vsize_j, cell_j = floorf(t_j).  A query
 *   is VALID when it lies below *n_queries, its batch id is in [0, batch) and cell_j is in [0, extent_j) on every
 *   axis (false for NaN).  Its CANDIDATES are the cells cell + o with |o_d| <= query_range[d], visited in ascending
 *   linear key: axis 0 outermost, the last axis innermost, every offset ascending.  A candidate is a HIT when it lies
 *   inside the grid, a LIVE row holds it (a row below *n_live with its batch index and coordinates in range; a
 *   coordinate held twice goes to the lowest row) and, with flag 1, d2 < r2 where, all in fp32 and every operation
 *   rounded on its own (no FMA), v_j being the candidate's coordinate:
 *     centre_j = (float(v_j) + 0.5f) * vsize_j + lo_j,  d_j = centre_j - q_j,
 *     d2 = (d_0 * d_0 + d_1 * d_1) + d_2 * d_2          (ndim 2: d_0 * d_0 + d_1 * d_1)
 *   The first nsample hits in visiting order are kept: rows[i, s] = the row of hit s, offsets[i, s, j] = its d_j,
 *   count[i] = min(hits, nsample).  Slots at or beyond count[i] hold row -1 and offsets 0, or, with flag 2 and
 *   count[i] > 0, slot 0 again.  An invalid query has count 0 and rows -1.
 *   A query belongs to a group of 1 .. 64 lanes which test the candidates of one round together and stop once nsample
 *   slots are taken.  With a rank map the caller vouches that the live rows are in ascending, unique key order; the
 *   unit of work is then a line of the window along the last axis (one or two words of the map, consecutive rows): one
 *   launch, ws may be NULL.  With rankmap = NULL the call builds the hash table of the index builders in ws and
 *   probes it per cell: a fill, the insert pass, the query pass.  Both forms return identical results for a
 *   key-ordered, duplicate-free level.  Requires n_cap * nsample < 2^31, at most 2^30 rows, and batch x grid within a
 *   63-bit key.
 *   spx_voxel_query_ws_bytes: scratch of the hash form (ranked = 0), monotone in n; 0 for ranked != 0 and for
 *   arguments that are refused.
 *
 *   spx_group_fwd: out[e, :] = vfeat[rows[e], :] for the entries e = i * nsample + s ([n, C] -> [n_cap, nsample, C],
 *   contiguous; SPX_F16 / SPX_BF16 / SPX_F32 / SPX_F64), zeros where rows[e] is outside [0, n).  The bits move
 *   unchanged.  Rows whose byte size is a multiple of 16 (and 16-byte aligned pointers) move as 16-byte pieces per
 *   lane, other widths element by element.  One launch, every output element written exactly once.
 *
 *   spx_group_bwd: the gradient with respect to the voxel rows over the TRANSPOSED list: offsets [n + 1] and list
 *   [n_cap * nsample] = spx_point_groups(ids = rows flattened, id_bytes 4, n_cap * nsample entries, num_voxels = n).
 *   dvfeat[v, :] = sum over e in list[offsets[v] .. offsets[v + 1]) of dout[e, :], in list order (ascending e), fp32
 *   accumulation (fp64 for SPX_F64) from zero, one round-to-nearest-even into the feature type; zeros for an empty
 *   group and for rows at or beyond *n_live.  No atomics, identical run to run; the walk of spx_interp_bwd.  One
 *   launch.
 * spx_group_fwd / _bwd on dirty buffers, unnamed rows and NaN / Inf: "What the row operators may be handed" (before the
 * misaligned add). */
size_t spx_voxel_query_ws_bytes(int n_cap, int nsample, int ndim, int n, int ranked);
int spx_voxel_query(const float *queries, int nfeat, const int32_t *batch_ids, int n_cap,
                    const int32_t *n_queries_dev, int ndim, const float *vsize, const float *coors_range,
                    const int32_t *indices, int n, const int32_t *n_live, int batch, const int *spatial_h,
                    const void *rankmap, size_t rankmap_bytes, const int *query_range, int nsample, float r2,
                    int flags, int32_t *rows, int32_t *count, float *offsets, void *ws, size_t ws_bytes,
                    spx_stream_t stream);
int spx_group_fwd(const void *vfeat, int n, const int32_t *rows, int n_cap, int nsample, int C, int dtype, void *out,
                  spx_stream_t stream);
int spx_group_bwd(const void *dout, int n_cap, int nsample, const int32_t *offsets, const int32_t *list, int n,
                  const int32_t *n_live, int C, int dtype, void *dvfeat, spx_stream_t stream);

/* ---- farthest-point sampling and ball query over raw points (csrc/sample.hip) -------------------------------
 * The keypoint stage of the point-voxel detectors (PV-RCNN, PV-RCNN++, Voxel R-CNN's raw-point source): keypoints are
 * chosen from the raw cloud by farthest-point sampling, and every keypoint collects the first `nsample` raw points
 * inside a radius -- the furthest_point_sample / ball_query extensions of pointnet2_stack.  The rows a ball query
 * returns are what spx_group_fwd / spx_group_bwd take, with the points as the "level".  Every call: the caller
 * allocates, nothing is read back, nothing synchronises, every grid depends on host-known sizes only (hipGraph-safe).
 * The argument checks that need no pointer come before any pointer is looked at.  No gradient with respect to
 * coordinates.
 *
 * SCENES.  points = fp32 [n_cap, nfeat], the first ndim (2 or 3) columns x, y, z.  offsets int32 [batch + 1] and list
 * int32 [n_cap] are spx_point_groups(ids = the points' batch ids, num_voxels = batch): the points of scene b are
 * list[offsets[b] .. offsets[b + 1]), in ascending point index; ids outside [0, batch) and rows at or beyond the
 * device point count given to spx_point_groups are in no scene.  A point is additionally INVALID when one of its
 * first ndim coordinates is not finite; an invalid point is never a sample and never a hit.  All distances are fp32
 * with every operation rounded on its own (no FMA):
 *     d2 = (d_0 * d_0 + d_1 * d_1) + d_2 * d_2          (ndim 2: d_0 * d_0 + d_1 * d_1)
 *
 *   spx_fps: num_samples = K in 1 .. 65536, the same for every scene.  Per scene: slot 0 is the lowest valid point
 *   index; every valid point keeps t[i], +inf at first; at each step, with c the last chosen point and d_j = p_j[i] -
 *   p_j[c], t[i] = d2 < t[i] ? d2 : t[i], and the next sample is the not-yet-chosen valid point with the largest t,
 *   ties to the LOWEST point index.  A chosen point stops being a candidate, so the indices of a scene are distinct
 *   (pointnet2 repeats an index once only duplicates are left; otherwise the sequences agree).  idx int32 [batch, K]
 *   = point indices, -1 in slots at or beyond count[b]; count int32 [batch] = min(valid points of b, K).
 *   One workgroup of 1024 lanes per scene, one barrier per step.  A scene of up to spx_fps_resident_points() points
 *   keeps coordinates and t in registers; a larger one streams 16-byte {x, y, z, t} records, staged in ws in scene
 *   order.  The tier is chosen in the kernel from the scene's own count.  One launch.
 *   spx_fps_ws_bytes: the scratch (16 bytes per point of n_cap); monotone in n_cap; 0 for refused arguments.
 *
 *   spx_ball_query: queries = fp32 [m_cap, q_nfeat], q_batch_ids = int32 [m_cap] or NULL (all scene 0), n_queries_dev
 *   = NULL or a device int32: rows at or beyond it are no queries.  A query is VALID when it lies below *n_queries,
 *   its batch id is in [0, batch) and none of its first ndim coordinates is NaN.  Its hits are the valid points of ITS
 *   scene with d2 < r2, d_j = p_j - q_j, visited in ASCENDING POINT INDEX; the first nsample (1 .. 128) are kept:
 *   rows int32 [m_cap, nsample] = point indices, count int32 [m_cap] = min(hits, nsample), out_offsets fp32 [m_cap,
 *   nsample, ndim] (or NULL) = d_j.  Slots at or beyond count hold -1 / 0, or, with flag 2 (pad = first) and count >
 *   0, slot 0 again.  An invalid query has count 0.  flags = 0 | 2.  r2 = the squared radius, computed by the caller
 *   in fp32, >= 0.  Requires m_cap * nsample < 2^31.  One lane per query, workgroups of 256 consecutive queries
 *   which walk the scenes of their queries in ascending order and stage that scene's points in LDS.  One launch. */
int spx_fps_resident_points(void);
size_t spx_fps_ws_bytes(int n_cap, int batch, int ndim);
int spx_fps(const float *points, int nfeat, int n_cap, int ndim, const int32_t *offsets, const int32_t *list,
            int batch, int num_samples, int32_t *idx, int32_t *count, void *ws, size_t ws_bytes,
            spx_stream_t stream);
int spx_ball_query(const float *queries, int q_nfeat, const int32_t *q_batch_ids, int m_cap,
                   const int32_t *n_queries_dev, const float *points, int nfeat, int n_cap, int ndim,
                   const int32_t *offsets, const int32_t *list, int batch, int nsample, float r2, int flags,
                   int32_t *rows, int32_t *count, float *out_offsets, spx_stream_t stream);

/* ---- sectorised keypoint sampling: segmented farthest-point sampling (csrc/sample.hip) ------------------------
 * PV-RCNN++'s sectorized_proposal_centric_sampling and pointnet2_stack's stack_farthest_point_sample: keep the points
 * near the first stage's RoIs, cut every scene into azimuth sectors, give each sector a share of K in proportion to
 * its points and sample every sector on its own -- batch * S workgroups on batch * S CUs, none waiting for another.
 * A SEGMENT is a group of spx_point_groups over the segment ids written here (num_voxels = batch * S); the sampling
 * rule, the validity of a point, d2 and the scratch are those of spx_fps.  Every call: the caller allocates, nothing
 * is read back, nothing synchronises, every grid depends on host-known sizes only (hipGraph-safe), no atomics.  The
 * argument checks that need no pointer come before any pointer is looked at.  All float32 operations are rounded on
 * their own (no FMA; sqrt correctly rounded).  The three launches are not counted by spx_launch_count (as the entries of
 * csrc/roi.hip and csrc/boxgrad.hip): its key inventory stays as it is.
 *
 *   spx_sector_ids: seg int32 [n_cap] = b * S + sector for a valid point of scene b, else -1.  A point is in no
 *   segment when it lies at or beyond *n_points_dev (NULL: n_cap), its batch id (batch_ids NULL: 0) is outside
 *   [0, batch), one of its first ndim coordinates is not finite, or the RoI filter turns it down.
 *   SECTOR, S = num_sectors in 1 .. spx_sector_max() = 64, about the centre (cx, cy): with a = -(x - cx), b = -(y - cy),
 *   boundary k < S has the direction (c_k, s_k) = (cos, sin)(2 pi k / S) -- computed in float64 and rounded to float32,
 *   exactly (1, 0) (0, 1) (-1, 0) (0, -1) where 4 k % S == 0: spx_sector_table writes the S pairs to a HOST array
 *   float [S, 2] -- and the half-turn bit h_k = (2 k >= S).  The point's half turn is 0 when b > 0 or (b == 0 and
 *   a > 0), else 1; it is at or past boundary k when half > h_k, or half == h_k and c_k * b - s_k * a >= 0; sector =
 *   max((boundaries at or past) - 1, 0); a == 0 and b == 0 is sector 0.  No transcendental function runs on the device.
 *   This is OpenPCDet's floor((atan2(y, x) + pi) / (2 pi / S)) but for two cases: a point on the negative x axis with
 *   y = +0 gets index S there (which its loop never visits: the point is dropped) and sector 0 here; the origin is
 *   sector 0 here, S / 2 there.
 *   ROI FILTER (roi_filter = 1; ndim 3): boxes fp32 [m_cap, box_nfeat >= 7] = (x, y, z, dx, dy, dz, heading);
 *   box_offsets int32 [batch + 1] and box_list int32 [m_cap] are spx_point_groups over the BOX batch ids with the
 *   device box count (boxes beyond it and ids outside [0, batch) are in no scene).  A box is additionally INVALID when
 *   one of its seven values is not finite or a size is not > 0.  With d_j = centre_j - p_j over the valid boxes of the
 *   point's scene, the NEAREST box is the one with the lowest d2 (< +inf), ties to the lowest box index; the point is
 *   kept when  sqrt(d2_nearest) < sqrt(d2 of (0.5 * dx, 0.5 * dy, 0.5 * dz) of the nearest) + radius  (radius finite,
 *   >= 0) -- OpenPCDet's sample_points_with_roi, its quirk included: only the nearest centre's size counts.  A scene
 *   without a valid box keeps nothing.  One lane per point, workgroups of 256 consecutive points which walk the scenes
 *   of their points and stage that scene's boxes in LDS, spx_sector_box_tile() = 128 at a time.  One launch (none for
 *   n_cap = 0).
 *
 *   spx_fps_quota: offsets int32 [batch * S + 1] = spx_point_groups over seg.  With n_k the size of segment k of a
 *   scene and n their sum:  quota = n == 0 ? 0 : min(n_k, (n_k * K + n - 1) / n)  in 64-bit integers (the ceiling of
 *   the segment's share of K = num_samples in 1 .. 65536), slot = the exclusive prefix of the quotas inside the scene,
 *   count[b] = their sum <= K + S - 1.  quota, slot int32 [batch * S], count int32 [batch].  A wave per scene.  One
 *   launch.
 *
 *   spx_fps_segments: spx_fps per segment with K read from the device.  Segment g of `groups` (offsets int32
 *   [groups + 1], list int32 [n_cap]) samples k = min(quota[g], max_quota, its valid points) points into
 *       idx[(g / groups_per_row) * row_stride + slot[g] + 0 .. k)              (slot NULL: 0)
 *   in sampling order, and count[g] = k.  idx int32 [groups / groups_per_row, row_stride] holds -1 wherever no segment
 *   writes (a fill launch in front); quota[g] and slot[g] are clamped so that no store leaves the row: with the
 *   quotas and slots of spx_fps_quota, groups_per_row = S and row_stride = K + S - 1 a row is packed, sector by sector,
 *   without holes below count[b].  With slot NULL, groups_per_row 1 and quota = K everywhere it is spx_fps.  max_quota
 *   in 1 .. 65536; groups a multiple of groups_per_row; rows * row_stride < 2^31.  One workgroup of 1024 lanes per
 *   segment, the tier chosen from the segment's own count; a segment without points or quota leaves before its first
 *   barrier.  ws: spx_fps_ws_bytes(n_cap, groups, ndim), needed for n_cap > spx_fps_resident_points().  Two launches. */
int spx_sector_max(void);
int spx_sector_box_tile(void);
int spx_sector_table(int num_sectors, float *table_h);
int spx_sector_ids(const float *points, int nfeat, const int32_t *batch_ids, int n_cap, const int32_t *n_points_dev,
                   int ndim, int batch, int num_sectors, float cx, float cy, int roi_filter, const float *boxes,
                   int box_nfeat, int m_cap, const int32_t *box_offsets, const int32_t *box_list, float radius,
                   int32_t *seg, spx_stream_t stream);
int spx_fps_quota(const int32_t *offsets, int n_cap, int batch, int num_sectors, int num_samples, int32_t *quota,
                  int32_t *slot, int32_t *count, spx_stream_t stream);
int spx_fps_segments(const float *points, int nfeat, int n_cap, int ndim, const int32_t *offsets, const int32_t *list,
                     int groups, const int32_t *quota, const int32_t *slot, int groups_per_row, int row_stride,
                     int max_quota, int32_t *idx, int32_t *count, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ---- k-nearest-neighbour query and inverse-distance weights over raw points (csrc/knn.hip) ------------------
 * The way back from few points to many, and grouping by nearest neighbours instead of by radius: three_nn +
 * three_interpolate of pointnet2's feature propagation (PointNet++, PointRCNN, 3DSSD, IA-SSD, the point heads of the
 * PV-RCNN family) and knn_query of pointops (Point Transformer grouping, unpooling interpolation, DGCNN-style edge
 * features).  The call returns tables the library already blends and gathers: rows + weights at width 4 or 8 are what
 * spx_interp_fwd / spx_interp_bwd take, rows at width k what spx_group_fwd / spx_group_bwd take, with the points as
 * the "level".  The caller allocates, there is no workspace, nothing is read back, nothing synchronises, the grid
 * depends on host-known sizes only (hipGraph-safe), and the argument checks that need no pointer come before any
 * pointer is looked at.  No gradient with respect to coordinates or weights.
 *
 *   spx_knn_query: SCENES, the validity of a point (below the device point count given to spx_point_groups, a batch id
 *   in [0, batch), its first ndim coordinates finite) and d2 are those of the section above; queries, q_batch_ids and
 *   n_queries_dev as spx_ball_query takes them.  A query is VALID when it lies below *n_queries, its batch id is in
 *   [0, batch) and its first ndim coordinates are FINITE (stricter than the ball query, which turns down NaN only).
 *   With d_j = p_j - q_j, the result of a valid query is the count = min(valid points of its scene, k) smallest
 *   candidates under the TOTAL ORDER (d2, point index), written in that order: equal distances go to the lower point
 *   index.  (A non-negative float orders as its bits: the 64-bit key d2 bits << 32 | index decides both fields with
 *   one compare.)  The result does not depend on the order in which points are visited, nor on how queries or points
 *   are arranged across scenes.  k in 1 .. spx_knn_max_k() = 64; width >= k is the row stride of every table:
 *       rows        int32 [m_cap, width]           point indices
 *       count       int32 [m_cap]
 *       dist2       fp32  [m_cap, width]           (or NULL) d2
 *       weights     fp32  [m_cap, width]           (or NULL) see below
 *       out_offsets fp32  [m_cap, width, ndim]     (or NULL) d_j
 *   Slots in [count, k) hold -1 / 0, or, with flag 2 (pad = first) and count > 0, slot 0 again with weight 0; slots in
 *   [k, width) always hold -1 / 0.  An invalid query has count 0.  flags = 0 | 2.
 *   WEIGHTS are pointnet2's, in fp32 with every operation rounded on its own (square root and division correctly
 *   rounded), eps finite and >= 0:
 *       r_s = 1 / (sqrt(d2_s) + eps)       norm = ((r_0 + r_1) + r_2) ... over s < count, in ascending slot
 *       w_s = r_s / norm
 *   Squared distances that overflow fp32 are outside the contract.  Requires m_cap * width < 2^31.  One lane per query,
 *   workgroups of 256 consecutive queries which walk the scenes of their queries in ascending order and stage that
 *   scene's points in LDS; a lane keeps its k best keys sorted in registers (lists of 4, 16 or 64 by k).  Brute force
 *   per scene: no spatial index.  One launch (none for m_cap = 0). */
int spx_knn_max_k(void);
int spx_knn_query(const float *queries, int q_nfeat, const int32_t *q_batch_ids, int m_cap,
                  const int32_t *n_queries_dev, const float *points, int nfeat, int n_cap, int ndim,
                  const int32_t *offsets, const int32_t *list, int batch, int k, int width, float eps, int flags,
                  int32_t *rows, int32_t *count, float *dist2, float *weights, float *out_offsets,
                  spx_stream_t stream);

/* ---- voxel pruning (csrc/select.hip) ---------------------------------------------------------------------
 * Keep the most important rows of a sparse tensor and drop, or process separately, the rest: the pruned down-sampling
 * blocks of SPS-Conv and VoxelNeXt, and every sparse head that keeps its top-scoring voxels.  Stands where a torch
 * composite would: abs().mean(1), topk (ties unspecified), boolean indexing (a count read back: not capturable), rows
 * that know nothing of dead rows and leave without a rank map.  Every call: the caller allocates, every grid depends on
 * host-known sizes only, nothing is read back except by spx_select_count, and the argument checks that need no pointer
 * come before any pointer is looked at.
 *
 * ROW SCORE.  spx_row_score: score[i] (fp32 [n]) from feat [n, C] (contiguous; SPX_F16 / SPX_BF16 / SPX_F32 / SPX_F64,
 * any C >= 1); -inf for rows at or beyond *n_live (NULL or a device int32).  One launch, no atomics, every element
 * written exactly once.
 *   SPX_SCORE_ABSMAX: the maximum of |feat[i, c]| (exact in any order), rounded to fp32 for SPX_F64.  A row with a NaN
 *   element scores a positive NaN, as under SPX_SCORE_ABSMEAN ("What the row operators may be handed", (c)).
 *   SPX_SCORE_ABSMEAN: the sum of |feat[i, c]| in fp32 (fp64 for SPX_F64), divided by C in that type, rounded once to
 *   fp32.  THE ORDER OF THE SUM is a function of C and the dtype alone.  With e = the element size in bytes:
 *     V = 16 / e when C * e is a multiple of 16, else 1         (elements of a piece)
 *     P = C / V                                                 (pieces of a row)
 *     G = the smallest power of two >= P, at most 64            (lanes of a row)
 *     acc[s] = 0 for s = 0 .. G - 1
 *     for s in 0 .. G - 1: for p = s, s + G, s + 2 G, ... < P: for j = 0 .. V - 1: acc[s] = acc[s] + |feat[i, p V + j]|
 *     for d = G / 2, G / 4, ..., 1: for s in 0 .. d - 1: acc[s] = acc[s] + acc[s + d]
 *     score[i] = acc[0] / C
 *   every addition rounded on its own.  A row whose bytes are a multiple of 16 moves as 16-byte pieces per lane when
 *   feat is 16-byte aligned (the rule of spx_collapse_fwd) and element by element otherwise -- in the same order.
 *
 * TOP-K FLAGS.  spx_topk_flags: keep (uint8 [n]) = 1 for exactly k live rows, 0 elsewhere.  A row is LIVE when it lies
 * below *n_live and, when `indices` (NULL, or int32 [n, ndim + 1]) is given, its batch index is inside [0, batch).
 * With `live` the number of live rows: k_abs >= 0 gives k = min(k_abs, live); k_abs < 0 gives k = (int)(ratio *
 * (double)live) with ratio in [0, 1] -- one IEEE fp64 multiply, truncated, computed on the device.  Scores are ordered
 * by the unsigned KEY = bits ^ (bits >> 31 ? 0xffffffff : 0x80000000): a total order on all fp32 bit patterns (-0.0
 * below +0.0, a positive NaN above +inf).  Kept: every live row whose key is above the k-th largest key T, and of the
 * live rows whose key equals T those with the LOWEST ROW INDEX, as many as are needed.  sel_dev (device int32 [4]) =
 * {live, k, T, ties taken}; k = 0 leaves T = 0xffffffff and ties = 0.  n = 0, k = 0 and k = live are legal.
 *   Radix select on the key, most significant 8-bit digit first: per digit a histogram pass (per-wave copies in LDS,
 *   merged with integer atomics, whose result does not depend on order) and a pick by one workgroup; then the tie
 *   rows are counted per workgroup, the counts scanned, and one flag pass ranks the tie rows by a block scan.
 *   Launches: a fill, 4 x (hist, pick), ties, its scan, flags (n = 0: the fill and the picks).
 *   spx_topk_ws_bytes: its scratch; 0 for n < 0.  Monotone in n.
 *
 * ROW SELECTION.  indices = int32 [n, ndim + 1], keep = uint8 [n] (nonzero = keep), invert = 0 or 1.  A row is LIVE
 * when it lies below *n_live, its batch index is inside [0, batch) and every coordinate inside [0, extent): the rule
 * of the collapse builder.  A row is SELECTED when it is live and (keep[i] != 0) != invert.  The selected rows are
 * compacted in ascending input row (a stable compaction):
 *     out_indices [n_out, ndim + 1]
 *     rows        [n]: the output row of each input row, -1 if the row is not selected or is cut
 *     src         [n_out]: the input row of each output row
 *   spx_select_ws_bytes: scratch of a build over n rows; 0 for n < 0 and for ndim outside [1, 4].  Monotone in n.
 *   spx_select_count: a fill, the blocks' counts, their scan, and the call's ONE D->H read (synchronises the stream):
 *   result_h [2] = {selected rows, live rows}.
 *   spx_select_fill: with the SAME arguments and ws, unchanged since the count, the scatter.  n_out = the count's
 *   result; a smaller n_out keeps the first n_out selected rows, the entries of out_indices and src beyond the selected
 *   rows are -1.
 *   spx_select_static: the static-shape form: room for n_out_cap rows, nothing read back (hipGraph-safe): a fill, count,
 *   scan, scatter.  n_out_dev [3] (device) = {found -- may exceed the cap --, 0, live = min(found, cap)}; selected rows
 *   beyond the cap are cut in row order (rows entry -1); out_indices and src past the live count are -1: the dead-row
 *   contract of spx_collapse_static and spx_union_static.
 *   RANK MAP.  rankmap = NULL, or a buffer of spx_rankmap_bytes(ndim, batch, spatial_h): the caller vouches that the
 *   live input rows are in ascending, unique key order.  A subset of such rows, taken in row order, is in ascending,
 *   unique key order itself, so _fill and _static leave the rank map of out_indices behind (spx_rankmap_from_sorted
 *   over the result: two more launches, no marks, no scan); `violation` (device int32 [1] or NULL) as there.
 *
 * FEATURE ROWS use kernels the library already has: out[r] = feat[src[r]] is spx_voxel_to_point with a zero fill, the
 * gradient din[i] = dout[rows[i]] is spx_union_add_bwd with one operand.  A row keeps its bits.
 * Dirty buffers, unnamed rows and NaN / Inf: "What the row operators may be handed" (before the misaligned add). */
int spx_row_score(const void *feat, int n, int C, int dtype, int op, const int32_t *n_live, float *score,
                  spx_stream_t stream);
size_t spx_topk_ws_bytes(long long n);
int spx_topk_flags(const float *score, const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch,
                   int k_abs, double ratio, uint8_t *keep, int32_t *sel_dev, void *ws, size_t ws_bytes,
                   spx_stream_t stream);
size_t spx_select_ws_bytes(int ndim, long long n);
int spx_select_count(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, const int *spatial_h,
                     const uint8_t *keep, int invert, void *ws, size_t ws_bytes, int *result_h, spx_stream_t stream);
int spx_select_fill(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, const int *spatial_h,
                    const uint8_t *keep, int invert, int n_out, int32_t *out_indices, int32_t *rows, int32_t *src,
                    void *rankmap, size_t rankmap_bytes, int32_t *violation, const void *ws, size_t ws_bytes,
                    spx_stream_t stream);
int spx_select_static(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, const int *spatial_h,
                      const uint8_t *keep, int invert, int n_out_cap, int32_t *out_indices, int32_t *rows,
                      int32_t *src, int32_t *n_out_dev, void *rankmap, size_t rankmap_bytes, int32_t *violation,
                      void *ws, size_t ws_bytes, spx_stream_t stream);

/* ---- voxel serialisation (csrc/serialize.hip) --------------------------------------------------------------
 * The rows of a sparse level ordered along space-filling curves and cut into fixed-size patches: what the serialised
 * point / voxel transformers (Point Transformer V3, OctFormer, FlatFormer-style blocks) do between the SubM layers
 * they keep for positional encoding.  Stands where a torch composite would: a Hilbert encoder written as a Python loop
 * over bits and axes, argsort on int64, a scatter for the inverse, bincount + cumsum, padding arithmetic with read-backs,
 * none of it aware of dead rows or a device-side live count.  Every call: the caller allocates, nothing is read back,
 * every grid depends on host-known sizes only (hipGraph-safe), and the argument checks that need no pointer come
 * before any pointer is looked at.  Every output is an integer or a moved row: a host loop reproduces it bit for bit.
 *
 * KEYS.  spx_curve_keys: indices = int32 [n, ndim + 1] (batch index first), ndim in [1, 4]; n_live = NULL or a device
 * int32; depth in [1, 16] = bits per axis; orders_h = HOST array of n_orders (1 .. 8) order codes SPX_ORDER_*; axes_h
 * = HOST array [ndim], a permutation of the spatial axes 0 .. ndim - 1 (axis a = index column a + 1): the coordinates
 * X[0 .. ndim) a curve takes, X[0] the most significant.  The _TRANS orders swap X[0] and X[1] (ndim = 1: no change).
 * keys = uint64 [n_orders, n]: key[k, i] = (batch << (ndim * depth)) | code_k(X).  Requires ndim * depth +
 * bit_length(batch) <= 63.
 *   SPX_ORDER_Z: bit b of X[j] lands at bit b * ndim + (ndim - 1 - j).
 *   SPX_ORDER_HILBERT: Skilling's AxesToTranspose (AIP Conf. Proc. 707, 2004) on X -- the inverse-undo loop from Q =
 *   2^(depth - 1) down to 2, then the Gray encode -- and the result interleaved as above.  The code of a cell at depth
 *   d - 1 is the code of any of its children at depth d shifted right by ndim.
 *   A row is DEAD when its batch index is outside [0, batch), a coordinate is outside [0, 2^depth), or it lies at or
 *   beyond *n_live: its key is all 64 bits set in every order (-1 when read as int64).  One launch, one thread per row.
 *
 * ORDERS.  spx_serialize: keys as above (key_bits = ndim * depth + bit_length(batch) bits in use, batch_shift = ndim *
 * depth); order int32 [n_orders, n]: order[k, t] = the row with the t-th smallest key of row k, equal keys in ascending
 * row (a stable LSD radix sort over exactly the key_bits low bits, 8- or 9-bit digits, three launches per digit), so
 * dead rows follow every live row in ascending row; inverse int32 [n_orders, n]: inverse[k, order[k, t]] = t, a full
 * permutation; offsets int32 [batch + 1]: offsets[b] = live rows with a batch index below b (a bisection of the first
 * order), offsets[batch] = live rows.  Keys of at most 32 bits are narrowed by one launch and sorted by the 32-bit
 * sort of spx_mask_argsort, the inverse then takes one launch for all orders; wider keys take the 64-bit passes, every
 * order in the same three launches per digit, whose last scatter writes the inverse.  n = 0 writes offsets only.
 *   spx_serialize_ws_bytes: its scratch; monotone in n, 0 for arguments that are refused (n < 0, n_orders outside
 *   [1, 8], key_bits outside [1, 63]).
 *
 * PATCHES.  spx_patch_plan: order = ONE row of the above, int32 [n]; K = patch_size >= 1; the layout has P_cap = n / K +
 * batch patches of K slots (an upper bound of the sum over scenes of ceil(c_b / K), c_b = offsets[b + 1] - offsets[b]).
 * Scene b starts on a patch boundary and fills ceil(c_b / K) patches; slot j < c_b of the scene holds order[offsets[b]
 * + j].  The tail slots of a scene's last patch hold -1 (SPX_PAD_MASK), or (SPX_PAD_BORROW) the row held K slots earlier
 * when c_b >= K and -1 otherwise.  Outputs: patch_rows [P_cap, K]; patch_rows_canon [P_cap, K] = the same with borrowed
 * slots as -1; row_slot [n] = the canonical slot of a row, -1 for a dead row; row_slot2 [n] = its one borrowed slot or
 * -1; patch_scene [P_cap] = batch index, -1 for patches not in use; n_patches_dev [1] = patches in use.  Two launches:
 * a prefix over the scenes by one workgroup, then one thread per slot; every element written exactly once.  Requires
 * P_cap * K < 2^31.  spx_patch_plan_ws_bytes: its scratch; 0 for arguments that are refused.
 *
 * ROWS.  Rows into patches and back are spx_voxel_to_point over patch_rows / row_slot (gradient of the way back:
 * over patch_rows_canon), with a zero fill.  spx_patch_rows_bwd is the gradient of the way in: g = [slots, C] (slots =
 * P_cap * K), g_feat[r, :] = g[row_slot[r], :] + g[row_slot2[r], :], the canonical term first, added in fp32 (fp64 for
 * SPX_F64) and rounded once; a row with one slot keeps that slot's bits, a dead row gets zeros.  16-byte pieces where
 * the row and the pointers allow, element by element otherwise.  One launch, no atomics, identical run to run. */
#define SPX_ORDER_Z 0
#define SPX_ORDER_Z_TRANS 1
#define SPX_ORDER_HILBERT 2
#define SPX_ORDER_HILBERT_TRANS 3
#define SPX_PAD_MASK 0
#define SPX_PAD_BORROW 1
int spx_curve_keys(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, int depth, int n_orders,
                   const int *orders_h, const int *axes_h, uint64_t *keys, spx_stream_t stream);
size_t spx_serialize_ws_bytes(int n, int n_orders, int key_bits);
int spx_serialize(const uint64_t *keys, int n, int n_orders, int key_bits, int batch, int batch_shift, int32_t *order,
                  int32_t *inverse, int32_t *offsets, void *ws, size_t ws_bytes, spx_stream_t stream);
size_t spx_patch_plan_ws_bytes(int n, int batch, int patch_size);
int spx_patch_plan(const int32_t *order, const int32_t *offsets, int n, int batch, int patch_size, int pad,
                   int32_t *patch_rows, int32_t *patch_rows_canon, int32_t *row_slot, int32_t *row_slot2,
                   int32_t *patch_scene, int32_t *n_patches_dev, void *ws, size_t ws_bytes, spx_stream_t stream);
int spx_patch_rows_bwd(const void *g, int slots, const int32_t *row_slot, const int32_t *row_slot2, int n, int C,
                       int dtype, void *g_feat, spx_stream_t stream);

/* ---- rotated boxes: corners, overlap, IoU and non-maximum suppression (csrc/box.hip) --------------------------
 * The iou3d_nms extension of OpenPCDet / mmdet3d: boxes_iou_bev, boxes_iou3d_gpu, its aligned form and nms_gpu -- the
 * rotated NMS every detector head ends in (SECOND, PointPillars, CenterPoint, VoxelNeXt, Voxel R-CNN, PV-RCNN), the
 * proposal layer of the two-stage heads and their target assignment.  nms_gpu copies its suppression mask to the host
 * for the sequential pass; here that pass is a kernel, so the step can sit inside a captured graph.  Every call: the
 * caller allocates, every grid depends on host-known sizes only (hipGraph-safe), nothing is read back, nothing
 * synchronises, and the argument checks that need no pointer come before any pointer is looked at.  Every fp32
 * operation is rounded on its own (no FMA; the divide correctly rounded), so a host loop reproduces every output bit
 * for bit from the same corners (tests/refbox.py).  No entry of this section has a gradient; aligned pairs have one
 * in the next section.
 *
 * CORNERS.  spx_boxes_to_corners: boxes fp32 [n, nfeat >= 7] = (x, y, z, dx, dy, dz, heading), z the centre;
 * n_boxes_dev NULL or a device int32.  bev fp32 [n, 4, 2], zrange fp32 [n, 2].  With c = cosf(heading), s =
 * sinf(heading), hx = dx * 0.5f, hy = dy * 0.5f, corner k = 0 .. 3 has (lx, ly) = (+hx, +hy), (-hx, +hy), (-hx, -hy),
 * (+hx, -hy) and lies at (x + (lx * c - ly * s), y + (lx * s + ly * c)): counter-clockwise.  zrange = (z - dz * 0.5f,
 * z + dz * 0.5f).  A box is VALID when it lies below min(*n_boxes, n), its seven numbers are finite and dx, dy, dz > 0;
 * an invalid box gets NaN in all ten outputs.  One launch (none for n = 0), every element written.
 *
 * A CORNER TABLE (bev, zrange) may as well be the caller's own: any four corners of a convex quad in either
 * orientation.  In every entry below a box is INVALID when it lies at or beyond the device count given for its table or
 * one of its eight corner coordinates is not finite (SPX_BOX_IOU_3D: or one end of its z range).  bev must be 16-byte
 * aligned, zrange 8-byte aligned.
 *
 * OVERLAP of the subject quad A with the quad B, in this order of operations:
 *   a(P) = the signed area sum over the vertices in order, a = a + (x_i * y_{i+1} - x_{i+1} * y_i) from a = 0;
 *   area(P) = |a| * 0.5f.  A quad with a < 0 is walked in reverse (3, 2, 1, 0) by everything below, its area included:
 *   clockwise corners give the bits of the same corners counter-clockwise.
 *   Bounding rectangles: overlap 0 when maxx(A) < minx(B), maxx(B) < minx(A), or the same in y.
 *   Sutherland-Hodgman: A clipped against the edges e = 0 .. 3 of B, edge a = B[e] -> b = B[e + 1]: ex = b.x - a.x,
 *   ey = b.y - a.y, d(p) = ex * (p.y - a.y) - ey * (p.x - a.x), p inside when d >= 0.  Walking the polygon p_0 ..
 *   p_{n-1} (j = i + 1, cyclic): p_i is emitted when inside; when p_i and p_j differ in that flag, t = d_i / (d_i -
 *   d_j) and p_i + t * (p_j - p_i) is emitted (x and y alike).  A ninth vertex of a pass is dropped.  Fewer than three
 *   vertices after a pass: overlap 0.
 *   inter = min(area(clipped), min(area(A), area(B))): an IoU never exceeds 1, a box with itself gives exactly 1.
 *   SPX_BOX_OVERLAP_BEV: inter.  SPX_BOX_IOU_BEV: inter / max((area(A) + area(B)) - inter, 1e-8f).
 *   SPX_BOX_IOU_3D: h = max(min(zmaxA, zmaxB) - max(zminA, zminB), 0), inter3 = inter * h, vol = area * (zmax - zmin),
 *   inter3 / max((volA + volB) - inter3, 1e-6f).  A pair with an invalid box gives 0.
 * The result is not symmetric in A and B to the last bit: the subject is the first argument.
 *   spx_boxes_overlap: out fp32 [m, n], out[i, j] = value(A_i, B_j); rows at or beyond *n_a_dev and columns at or
 *   beyond *n_b_dev (NULL: all exist) are written as 0: every element is written.  zrange_a / zrange_b may be NULL
 *   unless mode is SPX_BOX_IOU_3D.  One launch over (ceil(m / 16), ceil(n / 256)) workgroups (none for m * n = 0):
 *   lanes own consecutive columns, the 16 subjects of a tile are staged in LDS once, the two polygon buffers of the
 *   clip are per-lane LDS slots.  n <= 65535 * 256.
 *   spx_boxes_overlap_aligned: out fp32 [n], out[i] = value(A_i, B_i).  One launch.
 *
 * NMS.  spx_nms_rotated over a corner table bev [n, 4, 2] with scores fp32 [n], batch_ids / class_ids int32 [n] or
 * NULL (all scene 0 / one class).  A CANDIDATE is a valid box whose batch id is in [0, batch), whose score is not NaN
 * and, with use_score_thresh = 1, is above score_thresh.  The candidates of a scene are RANKED by score descending --
 * by the total order on the fp32 bits that spx_topk_flags uses, -0.0 below +0.0 -- equal scores by ascending index;
 * only the first pre_max of a scene take part (1 <= pre_max <= spx_nms_max_pre() = 16384, 1 <= post_max <= pre_max).
 * A candidate is KEPT if and only if no earlier-ranked kept candidate of its scene -- with class_ids: of its scene and
 * class -- has iou_bev(earlier, it) > thresh (strict; the earlier one is the subject).  A scene stops at post_max kept.
 *     keep   int32 [batch, post_max]   the kept boxes' indices in rank order, -1 behind them
 *     count  int32 [batch]
 * every element written on every call.  Launches:
 *   key      uint64 key = (scene << 32) | ~orderable(score), orderable = bits ^ (bits >> 31 ? 0xffffffff : 0x80000000);
 *            all bits set for a box that is no candidate
 *   sort     spx_serialize with n_orders = 1, key_bits = 32 + bit_length(batch), batch_shift = 32: the rank order
 *            (stable: ties to the lower index) and the scenes' offsets
 *   mask     for rank i of a scene and each 64-rank block jb >= i / 64 one 64-bit word, bit j - 64 jb set when j > i,
 *            the classes agree and the IoU is above thresh; layout [rows, W], W = ceil(min(pre_max, n) / 64), a row per
 *            (scene, rank).  Only the upper triangle is written and only it is read; a workgroup beyond its scene's
 *            candidates leaves at once.  The ballot of a wave over its 64 columns is the word of a row.
 *   reduce   one wave per scene; the removed set is W / 64 <= 4 words per lane (instances of 1, 2 and 4: up to 4096,
 *            8192, 16384 ranks).  Per 64-rank block: the block's removed word is broadcast, the diagonal words are held
 *            one per lane and resolved by a uniform loop over the ranks still standing (a lane broadcast each); then
 *            the rows of the block's kept ranks are ORed into the removed set.
 *   spx_nms_ws_bytes: the workspace (keys, order, offsets, the sort's scratch, the mask); monotone in its arguments, 0
 *   for arguments that are refused.  The workspace may be handed over dirty; ws must be 256-byte aligned.
 *   Measurement only: the option SPX_TEST_NMS_STAGES = 1 | 2 | 3 (spx_set_option) ends the call behind its key / sort /
 *   mask step and leaves keep and count unwritten (tools/box_probe.py times the prefixes against each other).
 * Not here: the axis-aligned nms_normal_gpu, more than 16384 candidates per scene (gradients of aligned pairs: the
 * next section; points in boxes: the one after it). */
#define SPX_BOX_OVERLAP_BEV 0
#define SPX_BOX_IOU_BEV 1
#define SPX_BOX_IOU_3D 2
int spx_boxes_to_corners(const float *boxes, int nfeat, int n, const int32_t *n_boxes_dev, float *bev, float *zrange,
                         spx_stream_t stream);
int spx_boxes_overlap(const float *bev_a, const float *zrange_a, int m, const int32_t *n_a_dev, const float *bev_b,
                      const float *zrange_b, int n, const int32_t *n_b_dev, int mode, float *out, spx_stream_t stream);
int spx_boxes_overlap_aligned(const float *bev_a, const float *zrange_a, const int32_t *n_a_dev, const float *bev_b,
                              const float *zrange_b, const int32_t *n_b_dev, int n, int mode, float *out,
                              spx_stream_t stream);
int spx_nms_max_pre(void);
size_t spx_nms_ws_bytes(int n, int batch, int pre_max);
int spx_nms_rotated(const float *bev, const float *scores, const int32_t *batch_ids, const int32_t *class_ids, int n,
                    const int32_t *n_boxes_dev, int batch, float thresh, int use_score_thresh, float score_thresh,
                    int pre_max, int post_max, int32_t *keep, int32_t *count, void *ws, size_t ws_bytes,
                    spx_stream_t stream);

/* ---- differentiable rotated IoU: value and gradients of aligned pairs, the corners backward (csrc/boxgrad.hip) ----
 * What a rotated-IoU regression loss trains through: mmcv's diff_iou_rotated_3d under mmdet3d's RotatedIoU3DLoss, the
 * IoU-aware heads, the IoU-guided second stages.  Two launches, the rules of the section above: the caller allocates,
 * host-sized grids, nothing read back, no launch counter.  Every fp32 operation is rounded on its own (no FMA, the
 * divide correctly rounded): tests/refboxgrad.py reproduces every output bit for bit from the same corners.
 *
 * PAIRS.  spx_boxes_iou_aligned_grad over two corner tables of n boxes each (bev [n, 4, 2], zrange [n, 2] or NULL in the
 * plane, device counts or NULL), mode SPX_BOX_IOU_BEV or SPX_BOX_IOU_3D, penalty SPX_BOX_PENALTY_NONE or _DIOU, grad_out
 * fp32 [n] or NULL (all 1).  Outputs, each NULL or written in every element: value [n], gbev_a [n, 4, 2], gz_a [n, 2],
 * gbev_b [n, 4, 2], gz_b [n, 2]: grad_out[i] times the derivative of value[i] with respect to the corners and the z
 * range of pair i.  With all four gradient pointers NULL the launch is a forward.  A pair with an invalid box (the
 * rule of the section above, the counts included) has value 0 and zero gradients.  One lane per pair.
 *   RECORDS A and B as above: counter-clockwise (reversed when the signed sum is negative), area, bounding rectangle.
 *   Gradients are computed per record corner k and written at the CALLER's index: 3 - k for a reversed quad.
 *   garea(P)_k = ((y_{k+1} - y_{k-1}) * 0.5f, (x_{k-1} - x_{k+1}) * 0.5f), indices cyclic.
 *   small = min(area(A), area(B)).  Rectangles apart: inter = 0, ginter = 0.  Else clip = the Sutherland-Hodgman area
 *   above, inter = min(clip, small), and
 *     clip > small (the clamp binds): ginter = garea of A when area(A) <= area(B), else garea of B; 0 for the other.
 *     otherwise the EDGE INTEGRAL, A's edges against B, then B's edges against A, ginter from 0: for k = 0 .. 3, edge
 *       p = P[k] -> q = P[k + 1]: t0 = 0, t1 = 1; for e = 0 .. 3 of the other quad, a = Q[e], ex, ey and d() as in
 *       the clip, dp = d(p), dq = d(q): both < 0: the edge is dead; one < 0: t = dp / (dp - dq), t0 = max(t0, t) when
 *       it is dp, else t1 = min(t1, t).  A live edge with t0 < t1 gives, with nx = q.y - p.y, ny = p.x - q.x, w1 =
 *       (t1 * t1 - t0 * t0) * 0.5f, w0 = (t1 - t0) - w1: g[k].x += nx * w0, g[k].y += ny * w0, g[k + 1].x += nx * w1,
 *       g[k + 1].y += ny * w1, in this order.  (Not a derivative of the clip: no polygon, nothing indexed at run time.)
 *   In the plane h = ha = hb = 1 and the floor is 1e-8f; in space hraw = min(zmaxA, zmaxB) - max(zminA, zminB), h =
 *   max(hraw, 0), ha = zmaxA - zminA, hb likewise, the floor 1e-6f.  i3 = inter * h, sa = area(A) * ha, sb = area(B) *
 *   hb (the plane: inter and the areas themselves), s = sa + sb, uraw = s - i3, u = max(uraw, floor), iou = i3 / u.
 *   uraw > floor: u2 = u * u, ci = s / u2, cs = i3 / u2; else (the floor binds: the U term carries no gradient) ci =
 *   1 / u, cs = 0.  go = grad_out[i] or 1; ki = go * ci, ks = go * cs; in space kin = ki * h, kh = ki * inter, kaa = ks *
 *   ha, kab = ks * hb, kha = ks * area(A), khb = ks * area(B); in the plane kin = ki, kaa = kab = ks.
 *     gA_k = kin * ginterA_k - kaa * gareaA_k, gB_k = kin * ginterB_k - kab * gareaB_k    (x and y alike)
 *     th = kh when hraw > 0 else 0; the top is A's when zmaxA <= zmaxB, the bottom A's when zminA >= zminB (ties: A)
 *     gzA = (kha - (bottom is A's ? th : 0), (top is A's ? th : 0) - kha), gzB likewise with khb and the complement
 *   SPX_BOX_PENALTY_DIOU: centres ((x0 + x2) * 0.5f, (y0 + y2) * 0.5f) of the records, in space (zmin + zmax) * 0.5f;
 *   dx, dy, dz = centre(A) - centre(B), rho2 = (dx * dx + dy * dy) + dz * dz; x0 = min(minxA, minxB), x1 = max(maxxA,
 *   maxxB), w = x1 - x0, v likewise in y, d = max(zmaxA, zmaxB) - min(zminA, zminB), c2 = (w * w + v * v) + d * d; c =
 *   max(c2, 1e-12f); value = iou - rho2 / c.  kr = go / c, kc = go * (rho2 / (c * c)) when c2 > 1e-12f else 0.  Then, in
 *   this order: corners 0 and 2 of A get - kr * dx in x and - kr * dy in y, those of B get +; in x, then in y, walking
 *   A's corners 0 .. 3 and then B's, the FIRST corner equal to the upper end gets + kc * (w + w) (y: v + v) and the
 *   first equal to the lower end gets - it; gzA -= kr * dz in both ends, gzB += it; + kc * (d + d) to the zmax of A
 *   when zmaxA >= zmaxB, else of B, and - it to the zmin of A when zminA <= zminB, else of B.  The penalty is computed
 *   for pairs whose rectangles are apart as well.
 *   With penalty 0 value has the bits of spx_boxes_overlap_aligned.
 *
 * CORNERS, BACKWARD.  spx_boxes_to_corners_bwd: boxes [n, nfeat >= 7] and n_boxes_dev as in spx_boxes_to_corners, gbev
 * fp32 [n, 4, 2], gzrange fp32 [n, 2] or NULL (zeros); gboxes fp32 [n, nfeat], every element written: columns beyond
 * the seventh 0, the row of an invalid box 0.  With c, s, lx, ly of the forward and (gx_k, gy_k) = gbev[k]: x = sum
 * gx_k, y = sum gy_k, dx = 0.5f * sum +-(gx_k * c + gy_k * s) by the sign of lx, dy = 0.5f * sum +-(gy_k * c - gx_k * s)
 * by the sign of ly, heading = sum (gy_k * (lx * c - ly * s) - gx_k * (lx * s + ly * c)), all over k = 0 .. 3 in order;
 * z = gzmin + gzmax, dz = (gzmax - gzmin) * 0.5f.  One launch, one lane per box.
 * Not here: GIoU and a minimum-area enclosing box, gradients of the [m, n] matrix forms, second derivatives, half
 * precision, a gradient through the NMS. */
#define SPX_BOX_PENALTY_NONE 0
#define SPX_BOX_PENALTY_DIOU 1
int spx_boxes_iou_aligned_grad(const float *bev_a, const float *zrange_a, const int32_t *n_a_dev, const float *bev_b,
                               const float *zrange_b, const int32_t *n_b_dev, int n, int mode, int penalty,
                               const float *grad_out, float *value, float *gbev_a, float *gz_a, float *gbev_b,
                               float *gz_b, spx_stream_t stream);
int spx_boxes_to_corners_bwd(const float *boxes, int nfeat, int n, const int32_t *n_boxes_dev, const float *gbev,
                             const float *gzrange, float *gboxes, spx_stream_t stream);

/* ---- points in rotated boxes: frames, the point-major and the box-major query (csrc/roi.hip) --------------------
 * The geometric test of the roiaware_pool3d / roipoint_pool3d extensions of OpenPCDet / mmdet3d: points_in_boxes_gpu
 * (foreground labels of keypoints and points, ground-truth sampling, "drop boxes with fewer than k points"), the
 * point stage of roipoint_pool3d (PointRCNN's second stage) and the point-to-cell stage of roiaware_pool3d (Part-A2's).
 * The pooling itself is spx_group_fwd / spx_group_bwd over rows and spx_collapse_fwd / spx_collapse_bwd over the
 * spx_point_groups of cells.  Every call: the caller allocates, every grid depends on host-known sizes only
 * (hipGraph-safe), nothing is read back, nothing synchronises, no atomics (identical run to run), and the argument
 * checks that need no pointer come before any pointer is looked at.  Every fp32 operation is rounded on its own, in
 * the order written (no FMA; the divide correctly rounded), so a host loop reproduces every output bit for bit from
 * the same frames (tests/refroi.py).  No gradient of any kind.  No launch counter.
 *
 * FRAMES.  spx_boxes_to_frames: boxes fp32 [n, nfeat >= 7] = (x, y, z, dx, dy, dz, heading), z the centre; n_boxes_dev
 * NULL or a device int32; ex, ey, ez host floats, finite and >= 0 (OpenPCDet's pool_extra_width / enlarge_box3d).
 * frames fp32 [n, 8] = (x, y, z, hx, hy, hz, c, s), 16-byte aligned: hx = dx * 0.5f + ex, hy = dy * 0.5f + ey, hz = dz
 * * 0.5f + ez, c = cosf(heading), s = sinf(heading).  A box is VALID by the rule of spx_boxes_to_corners: it lies
 * below min(*n_boxes, n), its seven numbers are finite and dx, dy, dz > 0 (before enlargement); an invalid box gets
 * eight NaNs.  One launch, one lane per box (none for n = 0), every element written.  A frame table may as well be
 * the caller's own.
 *
 * THE TEST of a point (px, py, pz), whose three coordinates must be finite, against a frame:
 *   sx = px - x;  sy = py - y;  lz = pz - z;  lx = sx * c + sy * s;  ly = sy * c - sx * s
 *   inside = |lz| <= hz && lx > -hx && lx < hx && ly > -hy && ly < hy
 * OpenPCDet's check_pt_in_box3d: inclusive in z, strict in the plane.  A frame with a NaN fails every comparison: an
 * invalid box contains nothing.
 *
 * POINT MAJOR.  spx_points_in_boxes: points fp32 [n_cap, nfeat >= 3] (x, y, z first), p_batch_ids int32 [n_cap] or
 * NULL (all scene 0), n_points_dev NULL or a device int32; frames [m_cap, 8]; box_offsets int32 [batch + 1] /
 * box_list int32 [m_cap]: the scene list over the BOX batch ids (spx_point_groups: scene b = box_list[box_offsets[b]
 * : box_offsets[b + 1]] in ascending box index; boxes at or beyond a device count and boxes with a foreign batch id
 * are in no scene).  out int32 [n_cap]: for every point the LOWEST box index of its own scene whose frame contains
 * it; -1 for no box, for a point with a coordinate that is not finite, at or beyond *n_points, or with a batch id
 * outside [0, batch).  Every element is written.  One lane per point, workgroups of 256 consecutive points that walk
 * the scenes of their points in ascending order (points may arrive in any scene order) and stage the frames of a
 * scene's boxes in LDS, spx_points_in_boxes_tile() = 128 at a time, read back as broadcasts; a lane that has its box
 * stops testing, a scene's remaining tiles are skipped once every lane of the workgroup is done.  One launch; n_cap =
 * 0 does nothing, m_cap = 0 runs no walk: one fill writes -1.
 *
 * BOX MAJOR.  spx_box_query: frames [m_cap, 8], b_batch_ids int32 [m_cap] or NULL, n_boxes_dev NULL or a device
 * int32; points as above with offsets int32 [batch + 1] / list int32 [n_cap], the scene list over the POINT batch ids
 * (points at or beyond a device count are not in it).  nsample in 1 .. spx_box_query_max_nsample() = 16384, m_cap *
 * nsample < 2^31.  Per box m, over the points of its scene in ASCENDING POINT INDEX:
 *     rows   int32 [m_cap, nsample]      the first nsample points inside it
 *     count  int32 [m_cap]               min(hits, nsample)
 *     hits   int32 [m_cap]               all points inside it, uncapped
 *     local  fp32 [m_cap, nsample, 3]    (lx, ly, lz) of each kept point: PointRCNN's canonical transform; or NULL
 *     cells  int32 [m_cap, nsample]      with a grid (ox, oy, oz), each in 1 .. 64 -- (0, 0, 0): none, cells NULL --
 *                                        wx = (hx + hx) / float(ox), ix = min(max(int((lx + hx) / wx), 0), ox - 1),
 *                                        likewise iy and iz, and the entry is the GLOBAL cell id m * (ox * oy * oz) +
 *                                        (ix * oy + iy) * oz + iz; needs m_cap * ox * oy * oz < 2^31
 * Slots at or beyond count hold -1 in rows and cells and 0 in local; with flags = SPX_ROI_PAD_FIRST and count > 0 they
 * repeat slot 0, with SPX_ROI_PAD_CYCLE and count > 0 slot s holds slot s % count (roipoint_pool3d).  A box that is
 * invalid (a NaN frame), at or beyond *n_boxes or with a batch id outside [0, batch) has count = hits = 0.  Every
 * element of every table given is written.  A box per wave, spx_box_query_waves() = 4 boxes per workgroup: the 64
 * lanes test consecutive entries of the scene's list, a ballot and the popcount of the lanes below give each hit its
 * slot, slots go straight to global memory (no per-lane lists, no scratch); the walk does not stop at nsample because
 * hits is the total.  With a pad flag a second launch, one lane per slot, writes the padded slots: it reads what other
 * lanes of the first launch stored, and the end of a kernel orders that.  Brute force per scene, no spatial index.
 * m_cap = 0 does nothing; n_cap = 0 runs no walk: one fill writes -1 / 0.
 *
 * WHAT THE KERNELS MAY BE HANDED.  Every output in any state (each element is written, none is read before it is
 * written); boxes, frames and points with NaN / Inf anywhere (an invalid box or point, as above -- never a fault,
 * never a hit); batch ids of any value; rows of boxes, points and ids at or beyond the device counts in any state
 * (unnamed rows are not read by the queries: the lists do not name them, and the frames kernel reads no box at or
 * beyond *n_boxes); offsets and list entries are clamped / checked, not trusted.
 * Not here: a fused RoI-aware kernel, a cap per cell, the points_in_boxes_all matrix, gradients, a spatial index. */
#define SPX_ROI_PAD_NONE 0
#define SPX_ROI_PAD_FIRST 2
#define SPX_ROI_PAD_CYCLE 4
int spx_box_query_max_nsample(void);
int spx_box_query_waves(void);
int spx_points_in_boxes_tile(void);
int spx_boxes_to_frames(const float *boxes, int nfeat, int n, const int32_t *n_boxes_dev, float ex, float ey, float ez,
                        float *frames, spx_stream_t stream);
int spx_points_in_boxes(const float *points, int nfeat, const int32_t *p_batch_ids, int n_cap, const int32_t *n_points_dev,
                        const float *frames, int m_cap, const int32_t *box_offsets, const int32_t *box_list, int batch,
                        int32_t *out, spx_stream_t stream);
int spx_box_query(const float *frames, const int32_t *b_batch_ids, int m_cap, const int32_t *n_boxes_dev,
                  const float *points, int nfeat, int n_cap, const int32_t *offsets, const int32_t *list, int batch,
                  int nsample, int flags, int ox, int oy, int oz, int32_t *rows, int32_t *count, int32_t *hits,
                  float *local, int32_t *cells, spx_stream_t stream);

/* ---- centre-head targets (csrc/center.hip; not part of the reference) ----------------------------------------------
 * The Gaussian heatmaps and index tables of the centre heads (CenterPoint, VoxelNeXt, TransFusion, DSVT, HEDNet,
 * SAFDNet): OpenPCDet's CenterHead.assign_target_of_single_head and VoxelNeXt's sparse twin, which walk the
 * ground-truth boxes in Python.  Every call: the caller allocates, nothing is read back, nothing synchronises, every
 * grid depends on host-known sizes only (hipGraph-safe), every output element is written exactly once by the call
 * that owns it, no atomics: identical run to run.  The argument checks that need no pointer come before any pointer is
 * looked at.  All float arithmetic is fp32, every operation rounded on its own (no FMA contraction), division and
 * square root correctly rounded: numpy float32 reproduces every table bit for bit (tests/refcenter.py).  No launch
 * counters.
 *
 * THE MAP.  W x H cells (x fastest), each 1 .. 2^23; num_classes = C class planes, 1 .. SPX_CENTER_MAX_CLASSES;
 * batch in 1 .. 65535; batch * C * H * W < 2^31.  box_offsets int32 [batch + 1] / box_list int32 [m_cap]: the scene
 * list over the BOX batch ids (spx_point_groups with the device box count: scene b = box_list[box_offsets[b] :
 * box_offsets[b + 1]] in ascending box index).
 *
 * RECORDS.  spx_box_centers: boxes fp32 [m_cap, nfeat >= 7] = (x, y, z, dx, dy, dz, heading); b_batch_ids int32
 * [m_cap] or NULL (all scene 0); class_ids int32 / int64 [m_cap] (class_bytes 4 / 8), 0-based planes, or NULL (all
 * class 0); n_boxes_dev NULL or a device int32.  Host parameters: voxel sizes vx, vy > 0, range minimum x0, y0,
 * stride > 0 (all finite), max_objs >= 1, 0 < min_overlap < 1, min_radius in 0 .. 2^20.  Per box:
 *     cx = ((x - x0) / vx) / stride, clamped to [0, W - 0.5];  cy likewise against y0, vy, H
 *     ix = (int)cx;  iy = (int)cy                                  (truncation)
 *     w = (dx / vx) / stride;  h = (dy / vy) / stride;  ov = min_overlap
 *     b1 = h + w;  c1 = ((w * h) * (1 - ov)) / (1 + ov);  r1 = (b1 + sqrt(b1 * b1 - 4 * c1)) / 2
 *     b2 = 2 * (h + w);  c2 = ((1 - ov) * w) * h;  r2 = (b2 + sqrt(b2 * b2 - 16 * c2)) / 2
 *     a3 = 4 * ov;  b3 = (-2 * ov) * (h + w);  c3 = ((ov - 1) * w) * h;  r3 = (b3 + sqrt(b3 * b3 - (4 * a3) * c3)) / 2
 *     ret = min(min(r1, r2), r3), NaN when one of them is;  radius = max((int)ret, min_radius)
 *   (CornerNet's gaussian_radius(h, w, ov) as OpenPCDet carries it.)  A box has a GEOMETRY when it lies below
 *   min(*n_boxes, m_cap), its seven numbers are finite, dx, dy, dz > 0 and |ret| < 2^20.  Its SLOT is its position among
 *   the boxes of its scene in the list -- every box of the scene below the device count, with a geometry or not -- or
 *   -1 when its batch id is outside [0, batch), it lies at or beyond the device count or the position is >= max_objs.
 *   A box TAKES PART when it has a geometry, a slot and a class in [0, C).  Outputs:
 *     center fp32 [m_cap, 2] (cx, cy), cell int32 [m_cap, 2] (ix, iy), radius int32 [m_cap]: zeros without a geometry
 *     cls int32 [m_cap]: the class plane of a box that takes part, else -1;  slot int32 [m_cap]
 *     box_index int32 [batch, max_objs]: the box in slot s of scene b, -1 past the scene's boxes
 *     mask int32 [batch, max_objs]: 1 when that box takes part;  inds int32 [batch, max_objs]: iy * W + ix, 0 where
 *     the mask is 0
 *   One launch, max(m_cap, batch * max_objs) lanes: a lane per box (its slot by a bisection in the scene's list) and a
 *   lane per table entry.  m_cap = 0 writes the tables only.
 *
 * DENSE.  spx_center_heatmap: heat fp32 [batch, C, H, W]; element (b, c, y, x) is the maximum, over the boxes of scene
 * b with cls = c and |x - ix| <= radius and |y - iy| <= radius, of
 *     expf(-(float)(ddx * ddx + ddy * ddy) / ((2.f * sigma) * sigma)),  sigma = (float)(2 * radius + 1) / 6.f
 * with the integers ddx = x - ix, ddy = y - iy (their sum of squares in 64 bits, converted once); 0 where no box
 * reaches.  The gather form: a workgroup per 16 x 16 patch of one class plane, a lane per cell; the scene's records are
 * staged spx_center_tile() = 128 at a time and compacted to the boxes of the class whose windows meet the patch; the
 * maximum stays in a register and is stored once.  One launch, no zero fill.  It reads cell, radius and cls only.
 *
 * SPARSE (2-D levels).  indices int32 [n_cap, 3] = (b, y, x); a row is LIVE when it lies below min(*n_live, n_cap), its
 * batch id is in [0, batch) and its cell inside W x H.  row_offsets int32 [batch + 1] / row_list int32 [n_cap]: the
 * scene list over indices[:, 0] (spx_point_groups with the device row count).
 *   spx_center_nearest: nearest int32 [m_cap] = for a box that takes part the live row of its scene with the least
 *   (bits of d2, row index), d2 = (float(vx) - cx)^2 + (float(vy) - cy)^2 with the x term first -- ties to the lowest
 *   row --, -1 for a scene without a live row and for a box that takes no part.  A box to a wave (four per workgroup),
 *   64-bit keys reduced across the wave.  A second launch, one lane per table entry, writes inds int32 [batch,
 *   max_objs] = the nearest row of the box in that slot (a global row index; 0 where mask is 0) and mask = box_mask
 *   && a nearest row exists, from box_index / box_mask of spx_box_centers.
 *   spx_center_heatmap_sparse: heat fp32 [n_cap, C]; element (i, c) of a live row is the maximum over the boxes of its
 *   scene with cls = c of expf(-d2 / ((2.f * sigma) * sigma)), sigma as above.  anchor = SPX_CENTER_ANCHOR_CENTER
 *   (VoxelNeXt's gt_center): d2 as in spx_center_nearest, the window centred on (ix, iy).  SPX_CENTER_ANCHOR_NEAREST:
 *   d2 = the integer squared distance to the cell of the box's nearest row, converted once, the window centred on
 *   that cell; a box without a nearest row draws nothing.  cutoff = SPX_CENTER_CUTOFF_WINDOW keeps the dense rule
 *   |.| <= radius on both axes; SPX_CENTER_CUTOFF_NONE (VoxelNeXt) lets a box reach every live row of its scene.  A
 *   row that is not live gets zeros.  A lane per row on the scene walk of the point queries (workgroups of 256
 *   consecutive rows walk the scenes of their rows in ascending order; rows may arrive in any scene order), eight
 *   class maxima in registers; more than eight classes walk once per group of eight.  One launch.
 *
 * WHAT THE KERNELS MAY BE HANDED.  Every output in any state; boxes with NaN / Inf anywhere; batch ids, class ids and
 * index rows of any value; rows at or beyond the device counts in any state (they are not read); offsets and list
 * entries are clamped / checked, not trusted.
 * Not here: gaussian_ratio, IoU-aware targets, 3-D heatmaps, half-precision heat, decoding, the losses, gradients. */
#define SPX_CENTER_MAX_CLASSES 64
#define SPX_CENTER_ANCHOR_CENTER 0
#define SPX_CENTER_ANCHOR_NEAREST 1
#define SPX_CENTER_CUTOFF_NONE 0
#define SPX_CENTER_CUTOFF_WINDOW 1
int spx_center_tile(void);
int spx_center_max_classes(void);
int spx_box_centers(const float *boxes, int nfeat, const int32_t *b_batch_ids, const void *class_ids, int class_bytes,
                    int m_cap, const int32_t *n_boxes_dev, const int32_t *box_offsets, const int32_t *box_list, int batch,
                    int W, int H, float vx, float vy, float x0, float y0, float stride, int num_classes, int max_objs,
                    float min_overlap, int min_radius, float *center, int32_t *cell, int32_t *radius, int32_t *cls,
                    int32_t *slot, int32_t *box_index, int32_t *mask, int32_t *inds, spx_stream_t stream);
int spx_center_heatmap(const int32_t *cell, const int32_t *radius, const int32_t *cls, int m_cap,
                       const int32_t *box_offsets, const int32_t *box_list, int batch, int W, int H, int num_classes,
                       float *heat, spx_stream_t stream);
int spx_center_nearest(const float *center, const int32_t *cls, const int32_t *b_batch_ids, int m_cap,
                       const int32_t *indices, int n_cap, const int32_t *n_live_dev, const int32_t *row_offsets,
                       const int32_t *row_list, int batch, int W, int H, const int32_t *box_index, const int32_t *box_mask,
                       int max_objs, int32_t *nearest, int32_t *inds, int32_t *mask, spx_stream_t stream);
int spx_center_heatmap_sparse(const float *center, const int32_t *cell, const int32_t *radius, const int32_t *cls,
                              const int32_t *nearest, int m_cap, const int32_t *box_offsets, const int32_t *box_list,
                              const int32_t *indices, int n_cap, const int32_t *n_live_dev, int batch, int W, int H,
                              int num_classes, int anchor, int cutoff, float *heat, spx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SPCONV_AMD_H_ */
