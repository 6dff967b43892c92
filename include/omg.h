/* omg.h — C-ABI of the MI355X-native octree-mg V-cycle (libomg.so).
 *
 * Drop-in boundary for the per-level box loops of the reference octree-mg
 * (FermiQ/octree-mg @ 2025-06-14).  The reference has no C boundary: its plug
 * points are Fortran procedure pointers called once per box
 * (mg%box_op / mg%box_smoother / mg%box_prolong, src/m_data_structures.f90:
 * 330-336, interfaces :381-407) and the per-level loops of src/m_multigrid.f90.
 * This header replaces those loops at LEVEL granularity: the host (the Fortran
 * drop-in m_multigrid in octree-mg_amd/fortran/, or the Python mirror in
 * octree-mg_amd/) hands over the mg_t tree once, and every per-level step
 * runs as HIP kernels over level-contiguous device arrays.
 *
 * Conventions
 *   - Plain C types only; every call returns 0 on success, nonzero on error
 *     with the message in omg_last_error() (the Fortran wrapper turns it into
 *     `error stop`, like the reference's error stops).
 *   - Box ids are the reference's 1-based ids; neighbour ids follow the
 *     reference encoding (>0 box, 0 = mg_no_box (refinement boundary),
 *     <0 = physical boundary / bc code).  Variables iv are 1-based
 *     (1 phi, 2 rhs, 3 old, 4 res, 5.. extra), src/m_data_structures.f90:43-65.
 *   - Box data is exchanged as the reference stores it: cc(0:nc+1,0:nc+1,
 *     0:nc+1) of one variable, Fortran column-major (i fastest).
 *   - One context per process/GPU; calls are stream-ordered on the context's
 *     stream and not re-entrant.  Multi-GPU: one rank per GPU, halos over
 *     RCCL (ncclSend/ncclRecv, xGMI), bootstrapped from omg_get_unique_id().
 */
#ifndef OMG_H
#define OMG_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct omg_ctx omg_ctx;

#define OMG_UNIQUE_ID_BYTES 128
#define OMG_DEVICE_NONE (-2)

/* Operators / smoothers / bc codes: same values as the reference
 * (src/m_data_structures.f90:14-37, 73-79). */
enum { OMG_LAPLACIAN = 1, OMG_VLAPLACIAN = 2, OMG_HELMHOLTZ = 3, OMG_VHELMHOLTZ = 4,
       OMG_AHELMHOLTZ = 5 };
enum { OMG_SMOOTHER_GS = 1, OMG_SMOOTHER_GSRB = 2 };
enum { OMG_BC_DIRICHLET = -10, OMG_BC_NEUMANN = -11, OMG_BC_CONTINUOUS = -12 };

const char *omg_last_error(void);

/* RCCL bootstrap: rank 0 calls this and broadcasts the bytes to all ranks
 * (replaces mg_comm_init's MPI set-up, src/m_communication.f90:14-35). */
int omg_get_unique_id(void *out /* OMG_UNIQUE_ID_BYTES */);

/* Loopback transport (testing the multi-rank path on ONE GPU): fills `out`
 * with an id that makes omg_ctx_create join an in-process group `tag` of
 * n_ranks contexts, one host thread each, exchanging halos by device copies
 * instead of RCCL (same plans, kernels and reduction orders). */
int omg_loopback_unique_id(long long tag, void *out /* OMG_UNIQUE_ID_BYTES */);

/* Host transport: fills `out` with an id that makes omg_ctx_create use the
 * caller's own host messaging instead of RCCL; omg_set_host_transport then
 * installs it.  For ranks that cannot use RCCL, above all several MPI ranks
 * sharing one GPU (RCCL refuses two ranks on one device): every exchange
 * stages its segments through pinned host memory and waits on the host.
 * Same plans, wire order, packing kernels and reduction orders as RCCL.  The
 * Fortran drop-in installs MPI here (m_multigrid.f90), which is the
 * reference's own transport (sort_and_transfer_buffers,
 * src/m_communication.f90:37-66; mpi_allreduce, src/m_multigrid.f90:232,255). */
int omg_host_unique_id(void *out /* OMG_UNIQUE_ID_BYTES */);
/* One grouped round: send_bufs[i] (send_counts[i] doubles) to send_peers[i],
 * receive recv_counts[i] doubles from recv_peers[i] into recv_bufs[i]; a
 * pair's messages arrive in the order they were sent (every rank makes the
 * same sequence of rounds).  Returns 0 on success. */
typedef int (*omg_host_exchange_fn)(void *user, int n_send, const int *send_peers, const long long *send_counts,
                                    const double *const *send_bufs, int n_recv, const int *recv_peers,
                                    const long long *recv_counts, double *const *recv_bufs);
/* MPI_Allgather of n doubles per rank into all (n_ranks * n, rank order). */
typedef int (*omg_host_allgather_fn)(void *user, const double *mine, int n, double *all);
int omg_set_host_transport(omg_ctx *ctx, omg_host_exchange_fn exchange, omg_host_allgather_fn allgather,
                           void *user);
/* Number of visible HIP devices (a rank count above it means ranks share a
 * GPU, where only the host transport works). */
int omg_device_count(int *n);

/* Create a context on HIP device `device` (device < 0: rank modulo the number
 * of visible devices; OMG_DEVICE_NONE: a plan-only context that builds the
 * host tables of omg_tree_setup and touches no device, for inspecting the
 * communication plans with omg_plan_transfer) for rank `rank` of `n_ranks`.  unique_id may be NULL
 * when n_ranks == 1.  Replaces the device side of mg_comm_init
 * (src/m_communication.f90:14-35). */
int omg_ctx_create(omg_ctx **ctx, int device, int rank, int n_ranks, const void *unique_id);
int omg_ctx_destroy(omg_ctx *ctx);

/* Hand over the mg_t tree (replaces the device side of mg_allocate_storage,
 * src/m_allocate_storage.f90:51-99): per-box arrays indexed by id-1
 * (children 8/box, neighbors 6/box, ix 3/box, rank 1/box), per-level arrays
 * indexed by lvl-lowest (box_size_lvl, dr 3/level) and, for every level and
 * list type t in {ids, leaves, parents, ref_bnds}, the slice
 * lists[list_off[4*(lvl-lowest)+t] .. list_off[4*(lvl-lowest)+t+1]).
 * Allocates n_vars variables for every box owned by this rank, zeroed. */
int omg_tree_setup(omg_ctx *ctx, int n_boxes, const int *lvl, const int *parent,
                   const int *children, const int *neighbors, const int *ix,
                   const int *rank, int lowest_lvl, int highest_lvl,
                   int first_normal_lvl, int box_size, const int *box_size_lvl,
                   const double *dr, const int *list_off, const int *lists,
                   int n_vars);

/* mg_set_methods equivalents (src/m_multigrid.f90:27-60; the operators'
 * *_set_methods: m_laplacian.f90:13-49, m_vlaplacian.f90:13-49,
 * m_helmholtz.f90:18-37, m_vhelmholtz.f90:19-49, m_ahelmholtz.f90:19-57;
 * lambda as helmholtz_set_lambda m_helmholtz.f90:39-46 and its v/a forms).
 * omg_set_smoother may be called between cycles with other values; the next
 * cycle uses them (the reference reads mg%n_cycle_down, n_cycle_up,
 * max_coarse_cycles and residual_coarse_* afresh every cycle).  A count of 0
 * means no smoothing on that leg; a negative count is stored as 0, which is
 * what the reference's zero-trip loops make of it. */
int omg_set_operator(omg_ctx *ctx, int op, double lambda);
int omg_set_smoother(omg_ctx *ctx, int smoother, int n_cycle_down, int n_cycle_up,
                     int max_coarse_cycles, double residual_coarse_abs,
                     double residual_coarse_rel);
int omg_set_subtract_mean(omg_ctx *ctx, int on);

/* Replicated coarse levels (no reference counterpart: a scaling option of
 * this library, call before omg_tree_setup).  With n_ranks > 1, the lowest
 * levels, as long as each holds at most max_cells cells and has neither leaves
 * nor refinement boundaries, are kept on EVERY rank instead of being split by
 * mg%boxes(:)%rank: the restriction into the highest such level is sent to all
 * ranks and the levels below it run without any exchange (the latency-bound
 * part of a multi-GPU V-cycle).  Results are bit-identical (every box computes
 * the same arithmetic; get_sum only reads leaves).  The host still sees its
 * own partition: omg_level_size / omg_download_level cover the boxes
 * mg_load_balance gave this rank, and omg_upload_level on a replicated level
 * is collective (every rank calls it, with its own boxes, possibly none).
 * Boundary tables (omg_set_bc_faces) must cover every box of a replicated
 * level.  0 (the default) = off.  omg_replicated_level gives the highest
 * replicated level (lowest_lvl - 1: none). */
int omg_set_coarse_replication(omg_ctx *ctx, long long max_cells);
int omg_replicated_level(omg_ctx *ctx, int *lvl);

/* Boundary conditions for variable iv (mg%bc(nb, iv), src/m_data_structures
 * .f90:235-242).  omg_set_bc_faces tabulates a boundary_cond callback:
 * face_off[(id-1)*6 + nb-1] = offset of nc*nc values in data (first
 * tangential index fastest) or -1; face_type = the bc type it returned.
 * Both first fill ghosts that a cycle deferred (under the condition that
 * held), then mark every level's ghosts stale; with several ranks they are
 * collective, like every other call that may fill. */
int omg_set_bc(omg_ctx *ctx, int iv, int nb, int bc_type, double bc_value);
int omg_set_bc_faces(omg_ctx *ctx, int iv, const long long *face_off,
                     const int *face_type, const double *data, long long n_data);

/* Number of boxes this rank owns at lvl (size(mg%lvls(lvl)%my_ids),
 * src/m_data_structures.f90:196-206). */
int omg_level_size(omg_ctx *ctx, int lvl, int *n_boxes, int *nc);

/* Bulk copy of variable iv of all my_ids boxes at lvl, in my_ids order,
 * (nc+2)^3 doubles per box as mg%boxes(id)%cc(:,:,:,iv) stores them
 * (src/m_data_structures.f90:209-221), host memory (blocking).
 * Multi-rank: an upload of phi (iv = 1) is collective, like every other call
 * that writes the device state: each rank calls it for the level, with its own
 * boxes, possibly none.  A stand-alone omg_fas_vcycle decides on every rank
 * alike, without communication, whether its ghost fill can be skipped; a phi
 * upload made on some ranks only would make that decision differ
 * (OMG_CHECK_COLLECTIVE=1 detects it: the decision is then also agreed over
 * the transport and a mismatch is an error). */
int omg_upload_level(omg_ctx *ctx, int lvl, int iv, const double *host);
int omg_download_level(omg_ctx *ctx, int lvl, int iv, double *host);

/* Stream-ordered dense device I/O (no reference counterpart; no staging
 * buffer, and no host synchronise except as the last paragraph says).  A dense window of level lvl's cell grid,
 * in DEVICE memory of the context's GPU: element (x,y,z), 0 <= x < n[0] etc.,
 * is dev[x*stride[0] + y*stride[1] + z*stride[2]] and is the cell whose
 * 0-based global index at lvl is lo + (x,y,z) (box ix, local i ->
 * (ix-1)*nc + (i-1)).  stride[0] must be 1, stride[1] >= n[0], stride[2] >=
 * stride[1]*n[1].  What moves: the interior cells of this rank's boxes at lvl
 * that fall inside the window.  Ghost slots are never read or written (a put
 * into rhs keeps what omg_phi_bc_store stored there); on put, cells outside
 * the window keep their values; on get, window elements that no box of this
 * rank covers keep theirs.  The window may be smaller than the level, cut
 * through boxes or reach outside the domain (no periodic wrap).
 * *n_cells (if non-NULL) = the cells copied, counted on the host from the box
 * table; a plan-only context (OMG_DEVICE_NONE) validates, counts and copies
 * nothing.
 * stream: the caller's hipStream_t (NULL: the null stream).  The copy runs on
 * omg_stream(ctx) after the work already queued on `stream`, and work queued
 * on `stream` afterwards runs after the copy.
 * State: omg_put_dense is a writer like omg_upload_level (pending work on phi
 * is applied first, derived copies of rhs are dropped, a put of phi makes the
 * level's ghosts stale and is collective in the same sense); it leaves the
 * ghost cells as they are, so after a put of phi they are those of the old
 * phi until the next fill.  omg_get_dense reads like omg_download_level, the
 * host's own boxes on a replicated level; omg_put_dense refuses a replicated
 * level (use omg_upload_level).  Errors (nothing is launched): a bad lvl, iv,
 * extent or stride, a NULL pointer with a non-empty window, a pointer that is
 * not device memory of the context's GPU.
 * Environment, read per call: OMG_DENSE_GENERIC=1 the per-cell kernel for
 * every box (A/B timing and cross-checks).
 * The clipping of the boxes against a window is kept per level for the four
 * most recent windows (a window: lo, n, stride, whether the base is 16-B
 * aligned, the switch above).  A call with one of them uploads nothing and
 * never waits on the host; a new window uploads its records from pinned
 * memory in stream order; a fifth distinct window on a level replaces the
 * oldest, and that call waits for the context's stream first. */
int omg_put_dense(omg_ctx *ctx, int lvl, int iv, const double *dev, const long long lo[3],
                  const long long n[3], const long long stride[3], void *stream,
                  long long *n_cells);
int omg_get_dense(omg_ctx *ctx, int lvl, int iv, double *dev, const long long lo[3],
                  const long long n[3], const long long stride[3], void *stream,
                  long long *n_cells);

/* The gradient of variable iv as dense windows in DEVICE memory (no reference
 * counterpart: the reference's users take cc(i+1) - cc(i-1) over
 * mg%boxes(id)%cc after mg_fill_ghost_cells_lvl, which is the definition
 * here).  lo, n, stride, stream and n_cells, the clipping and the plan-only
 * behaviour are exactly omg_get_dense's; the three component windows share
 * them.  dev[d] is the window of component d (0 x, 1 y, 2 z); a NULL dev[d]
 * skips that component.  For every interior cell (i,j,k) of this rank's boxes
 * inside the window, component d is
 *     (cc(+1 in d) - cc(-1 in d)) * f_d,   f_d = (0.5 * scale) / dr_d,
 * f_d computed once on the host in double with the level's dr: one
 * subtraction and one multiplication per value, no contraction (scale = -1
 * gives the field of a potential, signed zeros included).  cc is the stored
 * box with its face ghosts: i = 0 and nc+1 come from faces 1 and 2, j from
 * faces 3 and 4, k from faces 5 and 6; edge and corner ghosts are never
 * needed.  Window elements that no box of this rank covers keep their values.
 * fill != 0: the ghost cells of iv at lvl are filled first, as
 * omg_fill_ghost_cells_lvl fills them (physical, periodic, refinement-boundary
 * and remote ghosts); on several ranks the call is then collective like that
 * entry, made by every rank whatever its window.  For phi a fill that still
 * stands is skipped.  fill == 0: the ghosts are used as they stand (a variable
 * whose ghosts hold something on purpose, such as rhs after omg_phi_bc_store)
 * and the call is not collective.
 * State: the call reads like omg_get_dense (pending work on phi and rhs is
 * applied and deferred ghosts are filled before anything is read; the host's
 * own boxes on a replicated level); apart from the fill nothing of the state
 * changes, and a cycle after the call gives the bits it would have given
 * without it.
 * Stream ordering is omg_get_dense's; a call with a cached window never
 * waits on the host (a fill that exchanges over the loopback or host
 * transport, or runs a host refinement-boundary callback, waits as it does
 * anywhere).  The windows share the level's cache of four clippings with
 * omg_put_dense / omg_get_dense: the same records, "16-B aligned" being true
 * when every non-NULL base is.  OMG_DENSE_GENERIC=1: the per-cell kernel for
 * every box; both kernels give the same bits.
 * Errors (nothing is launched): a bad lvl, iv, extent or stride; all three
 * pointers NULL with a non-empty window; a non-NULL pointer that is not
 * device memory of the context's GPU or whose window reaches past the end of
 * its allocation; two non-NULL components whose windows (first to last
 * element) overlap.
 * Profiling families: dense_grad (the call), dense_grad_row (its tile kernel). */
int omg_get_dense_grad(omg_ctx *ctx, int lvl, int iv, double *const dev[3],
                       const long long lo[3], const long long n[3],
                       const long long stride[3], double scale, int fill,
                       void *stream, long long *n_cells);

/* Stream-ordered device block I/O for block-AMR hosts: the device equivalent
 * of the reference's coupling copies (coupling_amrvac/mod_multigrid_coupling.t:
 * mg_copy_to_tree :133-171, mg_copy_from_tree :206-234 and
 * mg_copy_from_tree_gc :238-267, three loops over the rank's leaf blocks).
 * Variable iv of a list of this rank's boxes, on any mixture of levels, <->
 * the caller's block pool in DEVICE memory of the context's GPU, with no host
 * copy and no host wait.
 * ids[n_boxes] and box_off[n_boxes] are host arrays; ids are the reference's
 * 1-based global box ids, in any order.  Element (i,j,k) of box q is
 *     dev[box_off[q] + (i-1) + (j-1)*stride[1] + (k-1)*stride[2]],
 * so box_off[q] is the offset, in doubles, of the box's interior cell (1,1,1).
 * The strides are shared by all boxes; stride[0] must be 1 and, with
 * m = nc_max + 2*ghost (nc_max: the largest box size listed), stride[1] >= m
 * and stride[2] >= stride[1]*m.
 * What moves: ghost == 0 the nc^3 interior cells 1 <= i,j,k <= nc; ghost == 1
 * additionally the six face-ghost layers (i = 0 and nc+1 with 1 <= j,k <= nc,
 * likewise for j and k), the ghost cells the device stores.  Edge and corner
 * elements of a block are never read on put and never written on get (as
 * mg_copy_from_tree_gc: "corner ghost cells not used/set").  Elements of dev
 * outside these cells keep their values, boxes not listed keep theirs.
 * Blocks of different boxes may interleave (blocks laid out as a dense grid
 * do, legitimately): overlap between them is the caller's responsibility.
 * *n_cells (if non-NULL) = the cells copied, sum of nc^3 + ghost*6*nc^2,
 * counted on the host; a plan-only context (OMG_DEVICE_NONE) validates, counts
 * and copies nothing.
 * stream: exactly omg_put_dense's ordering on the caller's hipStream_t.
 * State, omg_put_boxes: a writer like omg_upload_level (pending work on phi is
 * applied first, derived copies of rhs are dropped).  A put of phi (iv = 1)
 * makes the phi ghosts of EVERY level stale, since a rank cannot know which
 * levels its peers list, and is collective in the sense of an upload of phi:
 * every rank calls it, with n_boxes == 0 where it has nothing.  ghost == 0
 * leaves the ghost slots alone (a put into rhs keeps what omg_phi_bc_store
 * stored there); ghost == 1 writes the face slots as omg_upload_level does.
 * After omg_phi_bc_store those slots of rhs hold phi's boundary values: a put
 * of rhs with ghost == 1 (like an upload of rhs, a fill of rhs or
 * omg_subtract_mean of rhs with its ghosts) then makes the phi ghosts of every
 * level stale too, and is collective as a put of phi is.
 * A box on a replicated level is refused (use omg_upload_level).
 * State, omg_get_boxes: reads like omg_download_level (pending shifts are
 * applied, deferred ghosts filled and a pending res formed before anything is
 * read); on a replicated level only the host's own boxes are accepted.
 * fill != 0: the ghost cells of iv are filled first on every level, as
 * omg_fill_ghost_cells(ctx, iv) fills them (for phi a fill that still stands
 * is skipped per level); with several ranks the call is then collective,
 * whatever a rank lists.  fill == 0: the ghosts are used as they stand and the
 * call is not collective.  Apart from the fill nothing of the state changes: a
 * cycle after the call gives the bits it would have given without it.
 * Errors (nothing is launched, no state is touched): a bad iv, ghost or
 * stride, a negative n_boxes; NULL ids, box_off or dev with n_boxes > 0; an id
 * out of range, not owned by this rank or listed twice; |box_off| or a stride
 * beyond 2^40; a pointer that is not device memory of the context's GPU; a
 * block whose first or last touched element lies outside the pointer's
 * allocation (where hipMemGetAddressRange answers).
 * The records of a call (local box, level, offset; grouped by level, one
 * launch group per level that occurs) are cached on the context for the four
 * most recent lists; the key is n_boxes, ghost, the strides, whether the base
 * is 16-B aligned, and the contents of ids and box_off compared by value (the
 * switches below choose the kernel at launch: the records do not depend on
 * them).  A call with a cached list uploads nothing and never
 * waits on the host (a time loop repeats its list until a regrid); a new list
 * uploads its records from pinned memory in stream order; a fifth list
 * replaces the oldest, and that call waits for the context's stream first.
 * omg_tree_setup drops the cache.
 * Kernels: a tile kernel for 16^3 and 8^3 boxes, a per-cell kernel for every
 * other size, for a level of which fewer than 1536 boxes are listed and for a
 * get of interiors into rows with a gap between them (stride[1] > nc) of more
 * than 6144 * 16^3 cells, where it measured faster; both give the same bits.
 * Environment, read per call, for A/B timing and cross-checks:
 * OMG_BOXES_GENERIC=1 the per-cell kernel for every box; OMG_BOXES_TILE=1 the
 * tile kernel wherever it can serve; OMG_BOXES_ODD=8 / 16 the tile kernel's
 * variant for blocks that are not 16-B aligned (8-B accesses, or 16-B
 * accesses shifted by one cell, the default for a get with ghosts).
 * Profiling families: boxes_put, boxes_get (the call), boxes_put_tile,
 * boxes_get_tile (the tile kernel, per level). */
int omg_put_boxes(omg_ctx *ctx, int iv, int n_boxes, const int *ids, const double *dev,
                  const long long *box_off, const long long stride[3], int ghost,
                  void *stream, long long *n_cells);
int omg_get_boxes(omg_ctx *ctx, int iv, int n_boxes, const int *ids, double *dev,
                  const long long *box_off, const long long stride[3], int ghost, int fill,
                  void *stream, long long *n_cells);

/* The gradient of variable iv in block layout, in DEVICE memory: what a
 * block-AMR host computes after a solve (E = -grad phi, or the projection
 * B -= grad phi) from the blocks that mg_copy_from_tree_gc
 * (coupling_amrvac/mod_multigrid_coupling.t:236-267) hands it, here in one
 * pass from the stored boxes and their face ghosts, with no copy of the boxes
 * in between.  ids, box_off, stride, stream, the plan-only behaviour and the
 * ownership, range and "listed twice" checks are exactly omg_get_boxes's;
 * box_off[q] is the offset of interior cell (1,1,1) of box q and is shared by
 * the three component pools.  dev[d] is the pool of component d (0 x, 1 y,
 * 2 z); a NULL dev[d] skips that component.  Pools may interleave (the
 * slices [:, d] of one [n, 3, m, m, m] pool), as for omg_put_boxes.
 * With o(i,j,k) = box_off[q] + (i-1) + (j-1)*stride[1] + (k-1)*stride[2]:
 * centering == 0, cell-centred: for 1 <= i,j,k <= nc
 *     dev[d][o(i,j,k)] = (cc(+1 in d) - cc(-1 in d)) * f_d,
 *     f_d = (0.5 * scale) / dr_d,
 * omg_get_dense_grad's definition, rounding and signed zeros; stride[1] >= m
 * and stride[2] >= stride[1]*m with m = nc_max.
 * centering == 1, face-centred: for the index along d from 0 to nc and the
 * two other indices from 1 to nc
 *     dev[d][o(i,j,k)] = (cc(+1 in d) - cc(i,j,k)) * f_d,   f_d = scale / dr_d,
 * the difference across the face between the cells i and i+1 (along d) at
 * cell i's slot: a staggered array whose index i holds face i+1/2, so the
 * face 0 lies one element (d = 0), row (d = 1) or plane (d = 2) below the
 * interior; m = nc_max + 1 in the stride rule.
 * f_d is computed on the host in double with the dr of each box's level (a
 * list mixes levels): one subtraction and one multiplication per value, no
 * contraction.  cc is the stored box with its six face ghosts; the
 * refinement-boundary ghosts of a fill are the interpolation from the coarse
 * neighbour, so the differences over a leaf and its filled ghosts are the
 * composite gradient of the reference's users.  Edge and corner ghosts are
 * never read; pool elements outside the values named keep their bits, boxes
 * not listed keep theirs.
 * *n_cells (if non-NULL) = the values per component, counted on the host: sum
 * of nc^3, or of (nc+1)*nc^2 for face centring.
 * fill and state: exactly omg_get_boxes's (pending work is applied, deferred
 * ghosts are filled and a pending res is formed before anything is read;
 * fill != 0 fills iv on every level first and is collective on several ranks,
 * fill == 0 uses the ghosts as they stand; on a replicated level only the
 * host's own boxes are accepted; a cycle after the call gives the bits it
 * would have given without it).
 * Errors (nothing is launched, no state is touched): those of omg_get_boxes,
 * each non-NULL pool checked as its dev is, from the first to the last
 * touched element of the centring; a centering other than 0 or 1; all three
 * pointers NULL with n_boxes > 0; two non-NULL pointers that are equal.
 * The call shares the context's cache of four lists with omg_put_boxes /
 * omg_get_boxes (the same records; the centring is part of the key, "16-B
 * aligned" is true when every non-NULL base is): a cached list uploads
 * nothing and never waits on the host.
 * Kernels: a tile kernel for 16^3 and 8^3 boxes (16-B stores when every
 * base, box_off and stride is even, 8-B stores otherwise), a per-cell kernel
 * for every other size and where it measured faster: for a level of which
 * fewer than 512 (face centring) or 1536 (cell centring) boxes are listed,
 * and for cell centring into rows with a gap between them (stride[1] > nc)
 * of more than 2048 * 16^3 cells; both give the same bits.
 * OMG_BOXES_GENERIC=1 and OMG_BOXES_TILE=1 apply as they do to omg_get_boxes.
 * Profiling families: boxes_grad (the call), boxes_grad_tile (the tile
 * kernel, per level). */
int omg_get_boxes_grad(omg_ctx *ctx, int iv, int n_boxes, const int *ids,
                       double *const dev[3], const long long *box_off,
                       const long long stride[3], double scale, int centering,
                       int fill, void *stream, long long *n_cells);

/* The divergence of a vector field in block layout, in DEVICE memory, into
 * variable iv: the first step of a projection (rhs = div B; solve; B -= grad
 * phi), computed from the host's component pools in one pass with no scratch
 * pool in between: the mirror image of omg_get_boxes_grad.  ids, box_off,
 * stride, stream, the plan-only behaviour and the ownership, range and
 * "listed twice" checks are exactly omg_get_boxes_grad's.  dev[d] is the pool
 * of component d (0 x, 1 y, 2 z) of the field V; a NULL dev[d] skips that
 * component.  The pools are only read, so they may interleave, overlap or be
 * one and the same pointer.
 * With o(i,j,k) = box_off[q] + (i-1) + (j-1)*stride[1] + (k-1)*stride[2], for
 * every interior cell 1 <= i,j,k <= nc of every listed box variable iv is
 * overwritten with the sum of the terms t_d of the non-NULL components in the
 * order x, y, z: (t_x + t_y) + t_z, two components t_a + t_b, one alone t_d.
 * centering == 0, cell-centred: V_d(i,j,k) at dev[d][o(i,j,k)],
 *     t_d = (V_d(+1 in d) - V_d(-1 in d)) * f_d,   f_d = (0.5 * scale) / dr_d;
 * read are the block's interior and its six face-ghost layers (index 0 and
 * nc+1 along d, the two others in 1..nc); stride[1] >= m and
 * stride[2] >= stride[1]*m with m = nc_max + 2.
 * centering == 1, face-centred: dev[d][o(i,j,k)] is V_d on the face between
 * the cells i and i+1 along d, the layout omg_get_boxes_grad writes with
 * centering 1,
 *     t_d = (V_d(i,j,k) - V_d(-1 in d)) * f_d,     f_d = scale / dr_d;
 * read is the index along d from 0 to nc, the two others in 1..nc;
 * m = nc_max + 1 in the stride rule.  The face-centred divergence of the
 * face-centred gradient is the 7-point Laplacian the solver inverts.
 * f_d is computed on the host in double with the dr of each box's level (a
 * list mixes levels): one subtraction and one multiplication per term, then
 * the additions as written, no contraction, signed zeros as IEEE gives them.
 * Pool elements outside those named are never read: edges, corners, outer
 * ghost layers, a NULL component's pool.  The face-ghost slots of iv, every
 * other variable and boxes not listed keep their bits.
 * *n_cells (if non-NULL) = the cells written, sum of nc^3, counted on the
 * host.
 * State: exactly omg_put_boxes's with ghost == 0 (a writer: pending work is
 * applied first, derived copies of rhs are dropped; iv == 1 makes the phi
 * ghosts of every level stale and is collective in the same sense; a box on
 * a replicated level is refused).
 * Errors (nothing is launched, no state is touched): omg_get_boxes_grad's
 * list errors; a centering other than 0 or 1; all three pointers NULL with
 * n_boxes > 0; a non-NULL pool that is not device memory of the context's
 * GPU, or whose touched range leaves its allocation: from box_off - stride[d]
 * of the lowest block to the last interior element of the highest, plus
 * stride[d] for cell centring (stride[0] = 1).
 * The call shares the context's cache of four lists with the other block
 * entries (the same records; its centring is part of the key and distinct
 * from the copies' and the gradient's): a cached list uploads nothing and
 * never waits on the host.
 * Kernels: a per-cell kernel for every box size, which measured faster or
 * equal at every list length, and a tile kernel for 16^3 and 8^3 boxes that
 * reads the pools from global memory (16-B loads when every base, box_off
 * and stride is even, 8-B loads otherwise) and writes the stored box as
 * same-colour pairs with 16-B stores, kept for A/B timing and the tests'
 * cross-check under OMG_BOXES_TILE=1; both give the same bits.
 * OMG_BOXES_GENERIC=1 and OMG_BOXES_TILE=1 apply as they do to omg_put_boxes.
 * Profiling families: boxes_div (the call), boxes_div_tile (the tile kernel,
 * per level). */
int omg_put_boxes_div(omg_ctx *ctx, int iv, int n_boxes, const int *ids,
                      const double *const dev[3], const long long *box_off,
                      const long long stride[3], double scale, int centering,
                      void *stream, long long *n_cells);

/* omg_get_boxes_grad with an optional coefficient per component and an
 * optional accumulate: the flux c_face * grad(iv) of the operators with a cell
 * coefficient (D = -eps grad phi, u -= (1/rho) grad p, a heat flux), and the
 * last step of a projection (B -= grad phi) as a read-modify-write of the
 * host's pool.  ids, dev, box_off, stride, stream, n_cells, the plan-only
 * behaviour, the ownership, range and "listed twice" checks, the stride rule
 * (m = nc_max for cells, nc_max + 1 for faces), the elements touched per
 * centring and the rule that everything else of a pool keeps its bits are
 * exactly omg_get_boxes_grad's.
 * iv_coef[d] is the coefficient variable of component d: 0 none, otherwise a
 * variable 1..n_vars other than iv; iv_coef == NULL means {0, 0, 0}.
 * Let g be omg_get_boxes_grad's value of an element, the same f_d and the
 * same bits, (hi - lo) * f_d.  Then
 *     iv_coef[d] == 0:   v = g;
 *     centering == 1:    v = c * g,  c = ((2 * a_lo) * a_hi) / (a_lo + a_hi),
 * a the coefficient in the cells lo and hi of the face along d: the
 * reference's 2*a0*a/(a0+a) (src/m_vlaplacian.f90:84,152,
 * src/m_ahelmholtz.f90:152,229) evaluated left to right, symmetric in the two
 * cells, so two blocks that share a face get the same bits; it reads the
 * coefficient's face ghosts at the index 0 and nc+1 along d;
 *     centering == 0:    v = a(i,j,k) * g.
 * accumulate == 0: dev[d][o] = v; accumulate != 0: dev[d][o] = dev[d][o] + v,
 * one addition.  Every operation is rounded once, no contraction; signed
 * zeros, Inf and NaN as IEEE gives them; a_lo + a_hi == 0 is the caller's
 * affair.
 * State: iv is read exactly as omg_get_boxes_grad reads it, fill included
 * (collective on several ranks when set).  Each distinct coefficient variable
 * is read as omg_get_boxes(..., fill = 0) reads it: pending work is applied
 * and its ghosts are used as they stand, which is what the smoothers read.
 * Nothing else of the state changes: a cycle after the call gives the bits it
 * would have given without it.
 * Errors (nothing is launched, no state is touched): omg_get_boxes_grad's,
 * plus an iv_coef[d] out of range or equal to iv.  With accumulate each pool
 * is checked over the same range as without it.
 * The records and the cache key are the gradient's: a list that
 * omg_get_boxes_grad cached serves this entry and the other way round;
 * iv_coef, accumulate and scale are launch arguments, not part of the key.
 * Kernels: a tile kernel for 16^3 and 8^3 boxes (the gradient's staging of
 * iv in LDS; the coefficient read from the stored box by 16-B loads; 16-B or
 * 8-B loads ahead of the stores when accumulating), a per-cell kernel for
 * every other size and where it measured faster or nothing was measured: for
 * a level of which fewer than 512 boxes are listed, and for cell centring;
 * both give the same bits.
 * OMG_BOXES_GENERIC=1 and OMG_BOXES_TILE=1 apply as they do to
 * omg_get_boxes_grad.
 * Profiling families: boxes_flux (the call), boxes_flux_tile (the tile
 * kernel, per level). */
int omg_get_boxes_flux(omg_ctx *ctx, int iv, const int iv_coef[3], int n_boxes, const int *ids,
                       double *const dev[3], const long long *box_off, const long long stride[3],
                       double scale, int centering, int accumulate, int fill,
                       void *stream, long long *n_cells);

/* The hot path.  omg_fas_vcycle = mg_fas_vcycle (src/m_multigrid.f90:150-243);
 * highest_lvl < lowest_lvl means "not present".  omg_fas_fmg = mg_fas_fmg
 * (:84-147).  max_res is written when want_max_res (the optional argument). */
int omg_fas_vcycle(omg_ctx *ctx, int highest_lvl, int want_max_res, double *max_res,
                   int standalone);
int omg_fas_fmg(omg_ctx *ctx, int have_guess, int want_max_res, double *max_res);

/* Per-level steps, each the reference routine named (all in src/). */
int omg_apply_op(omg_ctx *ctx, int i_out);            /* mg_apply_op, m_multigrid.f90:439-456 */
int omg_restrict(omg_ctx *ctx, int iv);               /* mg_restrict, m_restrict.f90:72-80 */
int omg_restrict_lvl(omg_ctx *ctx, int iv, int lvl);  /* mg_restrict_lvl, m_restrict.f90:83-114 */
int omg_fill_ghost_cells(omg_ctx *ctx, int iv);       /* mg_fill_ghost_cells, m_ghost_cells.f90:120-128 */
int omg_fill_ghost_cells_lvl(omg_ctx *ctx, int lvl, int iv);
                                                      /* mg_fill_ghost_cells_lvl, m_ghost_cells.f90:131-175 */
int omg_prolong(omg_ctx *ctx, int lvl, int iv, int iv_to, int add);
                                                      /* mg_prolong + mg_prolong_sparse, m_prolong.f90:51-85,159-240 */
int omg_smooth_boxes(omg_ctx *ctx, int lvl, int n_cycle);
                                                      /* smooth_boxes, m_multigrid.f90:404-424 */
int omg_update_coarse(omg_ctx *ctx, int lvl);         /* update_coarse, m_multigrid.f90:347-384 */
int omg_correct_children(omg_ctx *ctx, int lvl);      /* correct_children, m_multigrid.f90:387-402 */
int omg_residual_lvl(omg_ctx *ctx, int lvl);          /* residual_box over my_ids, m_multigrid.f90:426-436 */
int omg_max_residual_lvl(omg_ctx *ctx, int lvl, double *out);
                                                      /* max_residual_lvl, m_multigrid.f90:296-311 */
int omg_get_sum(omg_ctx *ctx, int iv, double *out);   /* get_sum + MPI_Allreduce, m_multigrid.f90:253-294 */
int omg_subtract_mean(omg_ctx *ctx, int iv, int include_ghostcells);
                                                      /* subtract_mean, m_multigrid.f90:245-276 */
int omg_phi_bc_store(omg_ctx *ctx);                   /* mg_phi_bc_store, m_ghost_cells.f90:66-117 */

/* m_diffusion (src/m_diffusion.f90).  omg_set_rhs: its set_rhs (:144-159),
 * rhs = f1*phi + f2*rhs on the interior of this rank's leaves.
 * omg_diffusion_solve: diffusion_solve (:19-57) for op = OMG_HELMHOLTZ,
 * diffusion_solve_vcoeff (:63-101) for OMG_VHELMHOLTZ (coefficient in var 5),
 * diffusion_solve_acoeff (:108-142) for OMG_AHELMHOLTZ (vars 5..7), which
 * take diffusion_coeff = 1.  One implicit step of order 1 or 2 on phi: the
 * context's operator and lambda are left as the reference leaves them, then
 * FMG and up to 10 V-cycles until max_res.  *n_vcycles = V-cycles after the
 * FMG, *res = the last max residual.  Errors: "order should be 1 or 2",
 * "no convergence" (the reference's error stops). */
int omg_set_rhs(omg_ctx *ctx, double f1, double f2);
int omg_diffusion_solve(omg_ctx *ctx, int op, double dt, double diffusion_coeff, int order,
                        double max_res, int *n_vcycles, double *res);

/* m_free_space (src/m_free_space.f90).  omg_poisson_free_3d is
 * mg_poisson_free_3d (:36-214): on the first call (new_rhs must be set) and
 * whenever the FFT level changes, rhs is restricted down to the highest
 * uniform level with at most max_fft_frac of the unknowns and the free-space
 * Green's function of that grid is built (PSolver's createKernel, geocode
 * 'F', poisson_3d_fft/build_kernel.f90:55-199); with new_rhs the Poisson
 * problem is solved there by FFT convolution (PSolver, psolver_main.f90:
 * 91-556), phi gets Dirichlet values interpolated from that solution on every
 * physical face of every level (ghost_cells_free_bc + mg_phi_bc_store) and
 * the solution as initial guess (restricted down, prolonged up); then one FMG
 * (fmgcycle) or V-cycle runs unless the FFT level is the highest.  r_min:
 * mg%r_min of the domain (3 doubles); box_r_min: mg%boxes(id)%r_min, 3 per
 * box indexed by id-1, or NULL (then r_min + (ix-1)*nc*dr).  Operators other
 * than the Laplacian are refused ("mg_poisson_free_3d: laplacian operator
 * required"), as is a first call without new_rhs.  The transforms run on the
 * device (hipFFT); results agree with the reference at round-off.
 * omg_free_planes: the FFT level, nx (3 ints: the FFT level's domain + 2) and,
 * if planes holds cap >= 2*(nx2*nx3 + nx1*nx3 + nx1*nx2) doubles (else
 * nothing is copied), the six boundary planes bc_x0, bc_x1 (nx2*nx3 each),
 * bc_y0, bc_y1 (nx1*nx3), bc_z0, bc_z1 (nx1*nx2), first index fastest
 * (m_free_space.f90:163-171), for host copies of the boundary callback. */
int omg_poisson_free_3d(omg_ctx *ctx, int new_rhs, double max_fft_frac, int fmgcycle,
                        int want_max_res, double *max_res, const double *r_min,
                        const double *box_r_min);
int omg_free_planes(omg_ctx *ctx, int *fft_lvl, int *nx, double *planes, long long cap);

/* The communication plan of level lvl as built by omg_tree_setup: transfer
 * `which` (0 ghost faces, 1 restriction to lvl-1, 2 prolongation from lvl-1,
 * 3 refinement-boundary faces, 4 copies of the host's boxes of a replicated
 * level), direction dir (0 send, 1 receive); fills
 * min(cap, n) (peer, key) pairs in wire order.  Keys are the ordering keys of
 * sort_and_transfer_buffers (src/m_communication.f90:37-66): 6*id+nb for
 * faces, 8*parent+child slot for restriction, child id for prolongation,
 * box id for replicated-level copies. */
int omg_plan_transfer(omg_ctx *ctx, int lvl, int which, int dir, int cap, int *peers,
                      long long *keys, int *n_items, int *item_doubles);

/* The tables the block passes (k_gsrb3 / k_gsrb4) read level lvl through, as
 * built by omg_tree_setup: which 0 the column records (one per workgroup),
 * which 1 the coarse records of the correction form (one per column); the
 * layouts are described in octree-mg_amd/csrc/omg_kernels.h.  *n_cols records
 * of *rec_ints ints each, 0 where the level has none; recs gets them all if it
 * holds cap >= n_cols * rec_ints ints, else nothing (cap 0: the sizes only).
 * Host copies: the call works on plan-only contexts and changes no state.  On
 * a level split over ranks, the ranks agree on the coarse records after each
 * has built its own (all use them or none); a plan-only context joins no such
 * round and returns the ones it built. */
int omg_plan_columns(omg_ctx *ctx, int lvl, int which, int cap, int *recs, int *n_cols,
                     int *rec_ints);

/* The context's communicator (no reference counterpart; mg%n_cpu of
 * mg_comm_init, src/m_communication.f90:14-35, as the transport sees it):
 * *n_ranks = the ranks it joins (ncclCommCount for RCCL), *transport = one of
 * OMG_TRANSPORT_*. */
enum { OMG_TRANSPORT_NONE = 0, OMG_TRANSPORT_RCCL = 1, OMG_TRANSPORT_LOOPBACK = 2, OMG_TRANSPORT_HOST = 3 };
int omg_comm_info(omg_ctx *ctx, int *n_ranks, int *transport);

/* Stream / timing helpers for benchmarks. */
int omg_synchronize(omg_ctx *ctx);
void *omg_stream(omg_ctx *ctx);                 /* the hipStream_t all work runs on */
/* Custom refinement-boundary ghost cells: mg%bc(nb,iv)%refinement_bnd
 * (src/m_data_structures.f90:241, interface mg_subr_rb :364-378), which
 * fill_refinement_bnd calls instead of sides_rb (src/m_ghost_cells.f90:
 * 321-325).  fn runs on the host after every ghost fill of variable iv on a
 * level with refinement-boundary faces nb (the reference calls it once per
 * fill too), with n records: ids[n] (global box ids), nbs[n] (= nb),
 * cgc[n][nc*nc] (box_gc_for_fine_neighbor's coarse face, first index
 * fastest) and cc[n][(nc+2)^3] (the box's variable iv as
 * mg%boxes(id)%cc(:,:,:,iv) stores it: the interior and the other faces'
 * ghosts current, edges and corners 0).  fn sets the ghost cells of face nb
 * in cc; only those come back.  fn = NULL restores sides_rb.  A compat path:
 * each such fill waits for the GPU and copies the boxes both ways. */
typedef void (*omg_rb_fn)(void *user, int lvl, int iv, int n, const int *ids, const int *nbs, int nc,
                          const double *cgc, double *cc);
int omg_set_refinement_bnd(omg_ctx *ctx, int iv, int nb, omg_rb_fn fn, void *user);

/* Diagnostics (no reference counterpart): the number of times the host has
 * waited for one of the context's streams so far (a multi-rank stand-alone
 * V-cycle over RCCL waits only when max_res is requested, m_multigrid.f90:
 * 226-234; the loopback transport also waits to gather the periodic mean on
 * the host), and the priority of the halo-overlap stream (the greatest of
 * hipDeviceGetStreamPriorityRange). */
int omg_host_sync_count(omg_ctx *ctx, long long *n);
int omg_comm_stream_priority(omg_ctx *ctx, int *priority);
/* Per-kernel HIP-event timing (off by default): when on, every launch of the
 * named kernel families is bracketed by events on the stream it runs on, and
 * kept per family and per family@level.  "comm" / "comm_overlap" are the
 * RCCL (or loopback) rounds on the context stream / on the halo-overlap
 * stream, with cells = doubles received.
 * Environment switches read at omg_ctx_create ("0" = off):
 *   OMG_ROCTX=1  roctx ranges per level step (rocprofv3 --marker-trace);
 *   OMG_DEBUG=1  ghost faces start as signalling NaN and unstored edge /
 *                corner cells download as signalling NaN (the reference's
 *                DEBUG=1 -finit-real=snan, makerules.make:13-17);
 *   OMG_GRAPH=1  capture each cycle as a HIP graph.
 * Failure detection: a requested max residual (omg_fas_vcycle / omg_fas_fmg /
 * omg_max_residual_lvl / omg_poisson_free_3d, and diffusion_solve's loop)
 * that is NaN or Inf is an error, "non-finite residual", with max_res still
 * written; the reference's max() drops NaN (m_multigrid.f90:226-234). */
int omg_set_profiling(omg_ctx *ctx, int on);
int omg_kernel_stats(omg_ctx *ctx, const char *name, long long *launches,
                     double *total_ms, double *cells);
int omg_reset_stats(omg_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
