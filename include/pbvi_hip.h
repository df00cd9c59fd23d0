/*
 * pbvi_hip.h -- C-ABI of the MI355X (gfx950) PBVI alpha-vector backup engine.
 *
 * Drop-in boundary for ONE path of PimLb/POMDP_PBVI_Exploration: one call of
 * PBVI_Solver.backup (reference src/pomdp.py:1447-1524) plus the two kernels its
 * callers run on the same operands (ValueFunction.prune level 2, src/mdp.py:857-866;
 * compute_change's max_v b.alpha_v, src/pomdp.py:2165).  The reference has no FFI:
 * its GPU seam is CuPy array-module dispatch (`xp = cp.get_array_module(...)`,
 * src/pomdp.py:1482) over objects moved by Model.gpu_model (src/mdp.py:533-560),
 * ValueFunction.to_gpu (src/mdp.py:782-805) and BeliefSet.to_gpu
 * (src/pomdp.py:613-634).  Each entry point below names the reference statement(s)
 * it replaces.  Plain C types only; every array is C-order exactly as NumPy lays
 * the reference's arrays out.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - `dtype` selects the element type T of every `const void*` / `void*` array:
 *     PBVI_F32 -> float, PBVI_F64 -> double.  Indices are int32 (the binding narrows
 *     NumPy int64 after a range check).
 *   - Return value: 0 on success, negative pbvi_status otherwise; the message is
 *     available from pbvi_last_error() (thread-local).  The library itself never calls abort() or
 *     exit(); a GPU memory fault, however, is raised by the HSA runtime as a process abort that no
 *     library can intercept -- the engine validates every index array it is handed (ids, keys, actions,
 *     observations) on the host before a kernel can use it for exactly that reason.
 *   - Host pointers are owned by the caller and only read/written during the call.
 *     Device memory is owned by the handle.  A handle is not thread-safe.
 *   - Every call is synchronous: results are in the output buffers on return.
 */
#ifndef PBVI_HIP_H
#define PBVI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pbvi_engine pbvi_engine_t;

enum pbvi_status {
    PBVI_OK = 0,
    PBVI_EINVAL = -1,        /* bad argument (the reference asserts; binding raises ValueError) */
    PBVI_ENOMEM = -2,        /* host or hipMalloc OOM (binding raises MemoryError, which
                                PBVI_Solver.solve catches: src/pomdp.py:2399-2401) */
    PBVI_ERUNTIME = -3,      /* HIP runtime error */
    PBVI_EUNSUPPORTED = -4   /* configuration not supported by this build */
};

enum pbvi_dtype { PBVI_F32 = 0, PBVI_F64 = 1 };

/* Transition representation used for the Gamma projection (src/pomdp.py:1485-1491). */
enum pbvi_mode {
    PBVI_SPARSE = 0,   /* reachable-state padded-ELL SpMM (what the reference always does) */
    PBVI_DENSE = 1     /* densify T[A][S][S] on device and run the projection as |A| MFMA GEMMs */
};

enum pbvi_flags {
    PBVI_BELIEF_DOMINANCE = 1   /* backup(..., belief_dominance_prune=True), src/pomdp.py:1509-1515 */
};

/* Per-call instrumentation (kernel times from HIP events on the engine's stream). */
typedef struct pbvi_stats {
    double ms_total;        /* whole device-side backup, first kernel to last */
    double ms_project;      /* Gamma projection (K1) */
    double ms_score;        /* belief x Gamma score GEMM (K2) */
    double ms_argmax;       /* argmax over alpha-vectors + near-tie detection */
    double ms_refine;       /* fp64 refinement of near-ties (f32 engines) */
    double ms_action;       /* action values + argmax (K4) */
    double ms_assemble;     /* alpha' gather-sum (K3) */
    double ms_dominance;    /* belief-dominance test (K5), 0 if not requested */
    int64_t n_pairs;        /* B*A*O (belief, action, observation) triples */
    int64_t n_dead;         /* triples with P(o|b,a) == 0 (all scores exactly 0) */
    int64_t n_refined;      /* triples whose argmax was re-decided in fp64 */
    int64_t n_refined_actions; /* beliefs whose action argmax was re-decided in fp64 */
    int64_t n_unique;       /* distinct (action, best_alpha_ind[action]) keys = alpha' rows actually assembled */
    int64_t score_flops;    /* algorithmic 2*B*S*A*O*V of the score GEMM */
    int64_t score_flops_executed; /* MFMA flops actually issued (zero tiles skipped, pad tiles included) */
    int64_t score_tiles_dense;    /* 256x256x32 tile steps a dense GEMM of the padded shape would run */
    int64_t score_tiles_run;      /* tile steps actually run */
    int64_t project_flops;          /* dense mode: algorithmic 2*A*O*V*S*S of the projection GEMMs, else 0 */
    int64_t project_flops_executed; /* dense mode: MFMA flops issued by the projection GEMMs */
    int32_t split_k;        /* max K-chunks (partial slabs) per tile pair */
    int32_t formulation;    /* which operand was projected: 1 = alpha-vectors (Gamma), 2 = beliefs (pbvi_set_formulation) */
    int64_t n_refine_candidates; /* f32 engines: near-tie candidates listed over all refined triples (a triple that moves
                                    to the GEMM path -- every alpha row re-scored -- stops listing) */
    double ms_project_gemm;  /* dense mode: the batched projection GEMM kernel alone (ms_project also holds the
                                clears and the scale/copy pass around it); 0 in sparse mode */
    int32_t screened;        /* fp64 engines: 1 when the scores came from the fp32 screen (fp32 stream-K GEMM on rounded
                                copies of the operands, near-ties re-decided from the fp64 originals), 0 = pure fp64 */
    int32_t fused_projection; /* 1 when the score GEMM generated its Gamma tiles in the operand staging (R = 1, fp32
                                scoring, alpha-side formulation): ms_project then covers only the few projected rows */
    int32_t score_split;      /* 1 when the scores came from bf16 MFMAs on the three-term operand split (fp32 engines,
                                alpha-side formulation; pbvi_set_score_split), 0 = fp32 MFMAs */
    int32_t gamma_chunks;     /* alpha-side formulation: 1 = Gamma held whole (or compact: fused projection), n > 1 = Gamma
                                tiled over the alpha set into n chunks (pbvi_set_gamma_tiling); 0 = belief-side call.  In a
                                tiled call ms_project / ms_score are sums over the chunks and ms_argmax includes the
                                chunks' fold passes */
} pbvi_stats_t;

/* Library / device queries. */
int pbvi_version(void);
int pbvi_device_count(void);                 /* hipGetDeviceCount; 0 if no GPU */
const char* pbvi_last_error(void);

/*
 * Create an engine for one POMDP model on one device.  Replaces Model.gpu_model
 * (src/mdp.py:533-560): uploads and re-tiles the three tables the backup reads.
 *   reach_states [S][A][R] int32  = model.reachable_states            (src/mdp.py:194-201,296-335)
 *   rto          [S][A][O][R] T   = model.reachable_transitional_observation_table (src/pomdp.py:201-202)
 *   exp_reward   [S][A] T         = model.expected_rewards_table      (src/pomdp.py:251)
 * Model shapes the backup kernels cannot run are refused here with PBVI_EUNSUPPORTED (never by a launch in the middle of
 * a backup): A <= 256 and A * (1 + O) <= 65535.  S, O and R are otherwise bounded by memory only.
 */
int pbvi_engine_create(pbvi_engine_t** out, int device, int32_t S, int32_t A, int32_t O, int32_t R,
                       const int32_t* reach_states, const void* rto, const void* exp_reward,
                       int dtype, int mode);
void pbvi_engine_destroy(pbvi_engine_t* e);

/*
 * Device-resident alpha-vector set.  Replaces ValueFunction.to_gpu (src/mdp.py:782-805)
 * and the per-call re-stack of ValueFunction.alpha_vector_array (src/mdp.py:687-697).
 *   alpha [V][S] T, row-major.  set replaces the whole set; append adds rows at the end.
 */
int pbvi_alpha_set(pbvi_engine_t* e, const void* alpha, int64_t V);
int pbvi_alpha_append(pbvi_engine_t* e, const void* alpha, int64_t V_add);
int64_t pbvi_alpha_count(const pbvi_engine_t* e);

/*
 * Device-resident belief block.  Replaces BeliefSet.to_gpu (src/pomdp.py:613-634).
 *   beliefs [B][S] T, row-major, 1 <= B <= 65535 (PBVI_EUNSUPPORTED above; pbvi_beliefs_select has the same limit).
 */
int pbvi_beliefs_set(pbvi_engine_t* e, const void* beliefs, int64_t B);

/*
 * Device row stores.  The reference keeps every alpha-vector / belief on the GPU as its own CuPy array and
 * re-stacks them into a matrix on demand (ValueFunction.alpha_vector_array, src/mdp.py:687-697 -- an
 * O(V*S) copy after every extend; BeliefSet.belief_array, src/pomdp.py:541-550).  Here a row is uploaded
 * once (store_append returns the id of the first appended row, ids are consecutive) and the working
 * alpha set / belief block is then SELECTED by id, in the caller's order, entirely on the device.  The
 * order matters: argmax ties go to the lowest index, and ValueFunction.extend puts new vectors first
 * (src/mdp.py:773-774), so the selection must follow the host list order, not the upload order.
 * store_reset forgets all stored rows (ids restart at 0).
 *
 * pbvi_alpha_select keeps the selected set laid out with free rows in front of it: a later selection that is k new ids
 * followed by exactly the ids of the resident one -- what `new_value_function.extend(value_function)` produces after every
 * backup of a solve loop (src/pomdp.py:1521-1522) -- gathers those k rows only; a selection at most a quarter of the
 * resident one's size (compute_change's score of the rows an expansion added, src/pomdp.py:2141-2169) is placed beside it and
 * leaves it intact.  Results never depend on which of the paths was taken (same rows in the same order).
 * pbvi_alpha_layout reports it (tests, diagnostics): returns 1 when the working set is such an extendable selection, 0
 * otherwise (uploaded with pbvi_alpha_set / _append, or a small selection); *free_rows = rows still free in front of it,
 * *layouts = how many times a selection had to be gathered afresh so far.  Either pointer may be NULL.
 */
int64_t pbvi_alpha_store_append(pbvi_engine_t* e, const void* rows /* [n][S] T */, int64_t n);
int pbvi_alpha_select(pbvi_engine_t* e, const int32_t* ids /* [V] */, int64_t V);
int pbvi_alpha_layout(pbvi_engine_t* e, int64_t* free_rows, int64_t* layouts);
int pbvi_alpha_store_reset(pbvi_engine_t* e);
int64_t pbvi_belief_store_append(pbvi_engine_t* e, const void* rows /* [n][S] T */, int64_t n);
int pbvi_beliefs_select(pbvi_engine_t* e, const int32_t* ids /* [B] */, int64_t B);
int pbvi_belief_store_reset(pbvi_engine_t* e);

/*
 * One point-based backup on the resident alpha set and belief block
 * (src/pomdp.py:1485-1515).  Results stay on the device until fetched.
 */
int pbvi_backup_run(pbvi_engine_t* e, double gamma, int flags, pbvi_stats_t* stats /* may be NULL */);

/*
 * Copy the results of the last pbvi_backup_run to caller buffers (any may be NULL).
 * Destinations may be host memory or device memory of the engine's GPU (the copy kind
 * is resolved from the address), so the multi-GPU layer can land rows in its send buffer:
 *   out_alpha      [B][S] T        alpha_vectors  (src/pomdp.py:1506)
 *   out_action     [B] int32       best_actions   (src/pomdp.py:1505)
 *   out_best_alpha [B][A][O] int32 best_alpha_ind (src/pomdp.py:1495)
 *   out_keep       [B] uint8       dominating_vectors (src/pomdp.py:1512); all 1 if the
 *                                  run did not request PBVI_BELIEF_DOMINANCE
 */
int pbvi_backup_fetch(pbvi_engine_t* e, void* out_alpha, int32_t* out_action,
                      int32_t* out_best_alpha, uint8_t* out_keep);

/*
 * Deduplicated form of the same result (K6).  Beliefs with equal (best_action, best_alpha_ind[b,
 * best_action, :]) produce byte-identical alpha' rows, so the engine assembles one row per distinct
 * key -- a subset of the duplicates ValueFunction.__init__ removes by bytes (src/mdp.py:667-669), found
 * before any row is computed or moved.  U = pbvi_backup_unique_count():
 *   out_rows  [U][S] T     row u = alpha' of the first belief (in the caller's order) with that key
 *   out_index [B] int32    alpha'[b] == out_rows[out_index[b]]
 * Destinations may be host or device memory (pageable host destinations go through the engine's pinned bounce buffer,
 * here and wherever a comment below says "host or device").  pbvi_backup_fetch(out_alpha) expands this to [B][S].
 */
int64_t pbvi_backup_unique_count(const pbvi_engine_t* e);
int pbvi_backup_fetch_unique(pbvi_engine_t* e, void* out_rows, int32_t* out_index);

/*
 * Everything ValueFunction.__init__ needs of a backup (src/mdp.py:660-669 -- the `tobytes()` there is what makes
 * the reference's own backup timing include the device-to-host copy), in ONE staged transfer and one
 * synchronisation: out_rows [U][S] T, out_index [B], out_action [B], out_best_alpha [B][A][O], out_keep [B]; any
 * of them may be NULL.  Destinations in page-locked host memory (pbvi_host_alloc) are written by DMA directly;
 * pageable ones go through the engine's pinned bounce buffer.  This is the call SURVEY 8d's metric is timed on.
 */
int pbvi_backup_fetch_compact(pbvi_engine_t* e, void* out_rows, int32_t* out_index, int32_t* out_action,
                              int32_t* out_best_alpha, uint8_t* out_keep);

/*
 * pbvi_backup_run + pbvi_backup_fetch_compact in ONE call, with the rows leaving early.  The first maxima of the score
 * GEMM decide most beliefs' keys for good (the fp64 refinement re-decides near-ties only), so the distinct rows of that
 * provisional decision are assembled and written into out_rows by the device WHILE the refinement, the action stage and the
 * dedup run; the final keys are then matched against the provisional ones and only rows the refinement changed are appended.
 *   out_rows  [cap_rows][S] T   page-locked host memory (pbvi_host_alloc), cap_rows >= B; rows arrive in SLOT order
 *   out_slot  [B] int32         first U entries: row of distinct key u (order of first occurrence, as
 *                               pbvi_backup_fetch_compact lists them) is out_rows[out_slot[u]]
 *   out_index [B], out_action [B], out_best_alpha [B][A][O] (may be NULL), out_keep [B] (may be NULL): as
 *                               pbvi_backup_fetch_compact; alpha'[b] == out_rows[out_slot[out_index[b]]]
 *   *n_unique = U, *n_slots = rows written (>= U: provisional rows the refinement overturned stay behind, unreferenced)
 * Same results as the two calls (src/pomdp.py:1485-1506 + the tobytes() of src/mdp.py:667-669), bit for bit; where the
 * early path does not apply (fp64 scoring, belief-side formulation, belief-dominance test) the rows are copied at the end
 * and out_slot is the identity.
 */
int pbvi_backup_run_fetch(pbvi_engine_t* e, double gamma, int flags, pbvi_stats_t* stats, void* out_rows, int64_t cap_rows,
                          int32_t* out_slot, int32_t* out_index, int32_t* out_action, int32_t* out_best_alpha, uint8_t* out_keep,
                          int64_t* n_unique, int64_t* n_slots);

/*
 * Hashes of the U distinct rows of the last backup, out_hashes [U] uint64: sum_i bits(row, i) * (2 i + 1) mod 2^64 over
 * the row's fp32 / fp64 bit patterns.  ValueFunction.__init__ keys its dedup dictionary on `values.tobytes()`
 * (src/mdp.py:667-669) -- 120-240 KB copied and hashed per row; the host mirror keys it on this number instead (equality
 * is still decided on the bytes), computed where the rows are.
 */
int pbvi_backup_fetch_row_hashes(pbvi_engine_t* e, uint64_t* out_hashes);

/* Page-locked host memory for result buffers (hipHostMalloc / hipHostFree); NULL on failure.  The reference's
 * counterpart is CuPy's pinned-memory pool behind `cp.asnumpy` (src/mdp.py:806-831, ValueFunction.to_cpu). */
void* pbvi_host_alloc(size_t bytes);
void pbvi_host_free(void* p);

/*
 * The new alpha-vectors join the value function (ValueFunction.extend, src/mdp.py:763-779; append=True in
 * PBVI_Solver.backup, src/pomdp.py:1521-1522): append n of the last backup's distinct rows -- unique_idx[i] in
 * [0, U), in that order -- to the engine's alpha store, device to device.  Returns the store id of the first
 * appended row (ids are consecutive), or a negative error code.  The caller tags its AlphaVector objects with the
 * ids, so the next pbvi_alpha_select needs no upload of rows the engine computed itself.
 */
int64_t pbvi_backup_store_unique(pbvi_engine_t* e, const int32_t* unique_idx, int64_t n);

/*
 * Keys instead of rows (multi-GPU exchange).  The alpha' row of a belief is a function of its key
 * (a*, v*[a*, 0..O-1]) and of the replicated alpha set and model only (src/pomdp.py:1497-1506), so ranks exchange
 * keys -- (1+O) ints per distinct row -- and every rank assembles the rows it did not compute itself:
 *   pbvi_backup_fetch_unique_keys : out_keys [U][1+O] int32 of the last backup's U distinct rows (host or device)
 *   pbvi_assemble_rows            : out_rows [n][S] T (host or device) from n keys against the RESIDENT alpha set;
 *                                   byte-identical to the rows the producing rank holds.  1 <= n <= 65535.
 * Pageable host destinations go through the pinned bounce buffer, page-locked ones and device memory are written directly.
 */
int pbvi_backup_fetch_unique_keys(pbvi_engine_t* e, int32_t* out_keys);
/* Everything a rank contributes to the exchange in one int32 buffer of 1 + 3B + B(1+O) entries (host or device):
 *   [0] U | index [B] | actions [B] | keep [B] | keys of the U distinct rows, padded with zeros to [B][1+O]. */
int pbvi_backup_fetch_exchange(pbvi_engine_t* e, int32_t* out);
/* Same with per-sized sections, per >= B (= ceil(B_total / ranks) of a sharded run): 1 + 3 per + per (1+O) entries,
 * zeros behind the B valid ones, so every rank of a ragged split sends a message of the same length. */
int pbvi_backup_fetch_exchange_padded(pbvi_engine_t* e, int64_t per, int32_t* out);
int pbvi_assemble_rows(pbvi_engine_t* e, double gamma, int64_t n, const int32_t* keys, void* out_rows);
/* pbvi_assemble_rows whose rows also join the alpha store (ValueFunction.extend on every replica of a sharded
 * backup, src/pomdp.py:1521-1522 / src/mdp.py:763-779): returns the store id of the first of the n appended rows,
 * or a negative error code.  out_rows (host or device, [n][S] T; pageable host memory through the pinned bounce buffer)
 * may be NULL. */
int64_t pbvi_assemble_rows_store(pbvi_engine_t* e, double gamma, int64_t n, const int32_t* keys, void* out_rows);
/*
 * Host side of the key exchange of a belief-sharded backup (the step between the all-gather and
 * pbvi_assemble_rows_store; the reference has no counterpart: one device, Experiments/Olfactory Navigation/run_test.py:12).
 * all_meta: the `world` messages of pbvi_backup_fetch_exchange_padded in rank order, `stride` int32 apart
 * (stride >= 1 + 3 per + per key_width: a caller may carry its own trailer behind each message), HOST memory.
 * Rank r holds the beliefs [r per, min((r+1) per, n_total)).  Equal keys found by different ranks are ONE row.
 *   out_keys   [sum of the messages' counts][key_width]  the globally distinct keys in order of first occurrence
 *   out_index  [n_total]  position of each belief's key in out_keys     out_action / out_keep [n_total]
 * Returns the number of distinct keys, or a negative error code.  Pure host code: needs no engine and no device.
 * key_width (1 + O) >= 1 has no bound of its own: one message, per * (3 + key_width) + 1 int32 words, must fit int32.
 */
int64_t pbvi_exchange_merge(const int32_t* all_meta, int32_t world, int64_t stride, int64_t per, int32_t key_width,
                            int64_t n_total, int32_t* out_keys, int32_t* out_index, int32_t* out_action, uint8_t* out_keep);

/*
 * Device addresses of the last run's results, for the multi-GPU layer to hand to
 * RCCL (all-gather of the new alpha rows) without a host round trip.
 *   *d_alpha [B][S] T (row stride S), *d_action [B] int32, *d_keep [B] uint8.
 */
int pbvi_backup_device_results(pbvi_engine_t* e, void** d_alpha, int32_t** d_action, uint8_t** d_keep);

/*
 * Convenience: the reference seam in one call = beliefs_set + backup_run + backup_fetch
 * (PBVI_Solver.backup(model, belief_set, value_function, ...) before ValueFunction dedup).
 */
int pbvi_backup(pbvi_engine_t* e, const void* beliefs, int64_t B, double gamma, int flags,
                void* out_alpha, int32_t* out_action, int32_t* out_best_alpha, uint8_t* out_keep,
                pbvi_stats_t* stats);

/*
 * ValueFunction.prune(level=2) on the resident alpha set (src/mdp.py:857-866):
 *   keep[i] = 1 iff no other row j has alpha[j][s] >= alpha[i][s] for every s.
 */
int pbvi_prune_dominated(pbvi_engine_t* e, uint8_t* keep /* [V] */);

/*
 * The same prune from the pairs that involve a new row only (two launches of k_dominated_rect: all x new, new x old):
 *   keep[i] == 1  iff  (is_new[i] ? 0 : 1) + #{j : (is_new[i] || is_new[j]) and alpha[j][s] >= alpha[i][s] for every s} == 1
 * (j ranges over every resident row, i itself included; the comparison is the one of pbvi_prune_dominated, so a row that
 * holds a NaN dominates nothing and is dominated by nothing, itself included).
 * PRECONDITION, NOT CHECKED: the rows with is_new[i] == 0 are free of domination among themselves -- the survivors of an
 * earlier pbvi_prune_dominated / pbvi_prune_dominated_masked on this engine, or any subset of them.  Then keep equals
 * what pbvi_prune_dominated returns for the same rows, bit for bit, from 2*V*dV - dV*dV pair tests instead of V*V.  When
 * it does not hold the result is exactly the formula above: a pair of two old rows is never looked at.
 * An all-ones is_new is the full prune; an all-zeros is_new keeps every row and launches nothing.
 *   is_new [V] uint8 (non-zero = new), keep [V] uint8; host memory.  PBVI_EINVAL when either is NULL or no alpha set is
 *   resident, PBVI_EUNSUPPORTED above 262140 alpha-vectors (as pbvi_prune_dominated), PBVI_ENOMEM as everywhere
 *   (pbvi_engine_after_oom).
 */
int pbvi_prune_dominated_masked(pbvi_engine_t* e, const uint8_t* is_new /* [V] */, uint8_t* keep /* [V] */);

/*
 * max_v b.alpha_v over the resident alpha set for the resident belief block
 * (compute_change, src/pomdp.py:2165-2166; also the |V|-limiter scan :2349-2352).
 *   out_value [B] double, out_index [B] int32 (first max), either may be NULL.
 */
int pbvi_value_max(pbvi_engine_t* e, double* out_value, int32_t* out_index);

/*
 * One-step lookahead values of the resident belief block over the working alpha set: the quantity the backup's action
 * stage maximises (src/pomdp.py:1485-1506: Gamma :1485-1491, best_alpha_ind :1495, the per-action sums :1497-1505), for
 * EVERY (belief, action), exact in fp64 whatever the engine's type (an fp32 engine reads its fp32 tables, alpha rows and
 * beliefs and sums in fp64):
 *   Q[b][a] = b . ER[:,a] + gamma * sum_o max_v b . Gamma[a,o,v,:]
 *           = sum_s b[s] * ( ER[s,a] + gamma * sum_o sum_r RTO[s,a,o,r] * alpha[best_v[b,a,o]][rs[s,a,r]] )
 * with best_v[b,a,o] = first argmax_v b . Gamma[a,o,v,:] decided by the backup's own scoring, argmax and near-tie
 * refinement stages (every setting of pbvi_set_formulation, pbvi_set_f64_screen, pbvi_set_score_split,
 * pbvi_set_fused_projection and pbvi_set_gamma_tiling applies as it does to pbvi_backup_run: a Gamma-tiled call WORKS and
 * returns what the untiled call returns).  An observation that is impossible for (b, a) adds 0.  A one-step lookahead
 * policy executes a*(b) = argmax_a Q[b][a].
 *   out_q      [B][A] double, caller's belief order           (required: NULL gives PBVI_EINVAL)
 *   out_action [B] int32, may be NULL: the first maximum over a of the out_q row being returned, so
 *              out_action[b] == argmax_a out_q[b][:] holds EXACTLY, by construction (np.argmax semantics)
 *   out_best_v [B][A][O] int32, may be NULL: best_alpha_ind (src/pomdp.py:1495)
 * The sums run over each belief's non-zero 32-state tiles in a fixed order without atomics: the same bits on every run, and
 * the same bits from every pipeline setting that decides the same best_v.  No row is deduplicated, assembled or moved.
 * The belief block, the alpha set and both row stores are left as they were: a later pbvi_backup_run / pbvi_value_max
 * returns what it would have returned without this call.  The stage buffers of the backup are re-used, however: the
 * results of an EARLIER pbvi_backup_run can no longer be fetched afterwards (the fetches report that no result is resident).
 * PBVI_EINVAL without a resident belief block or alpha set (as pbvi_backup_run); PBVI_EUNSUPPORTED, with a
 * pbvi_last_error text, on a PBVI_DENSE engine.
 */
int pbvi_q_values(pbvi_engine_t* e, double gamma, double* out_q /* [B][A] */, int32_t* out_action /* [B], may be NULL */,
                  int32_t* out_best_v /* [B][A][O], may be NULL */);

/*
 * The same maxima for rows [0, n) of the BELIEF STORE (pbvi_belief_store_append / pbvi_belief_walk order) against the
 * working alpha set, with the store itself as the GEMM operand: nothing is gathered or sorted and the zero maps and
 * tile lists of rows scored before are kept.  compute_change (src/pomdp.py:2141-2169) scores the whole accumulated
 * belief set after every backup; that set only grows.  out_value / out_index: [n] (either may be NULL), store order.
 */
int pbvi_value_max_store(pbvi_engine_t* e, int64_t n, double* out_value, int32_t* out_index);
/*
 * max_v b.alpha_v of the beliefs of the last pbvi_backup_run against the alpha set it ran on, out_value [B] in the
 * caller's order: what compute_change (src/pomdp.py:2165) asks for next about exactly these beliefs and that set.
 * In the belief-side formulation the beliefs ride along as extra rows of the score GEMM (they fit its row padding), so
 * the values cost one row-max kernel.  fp32 engines: the GEMM's maxima (as with pbvi_set_value_max_exact(0)); f64
 * engines: the same sums pbvi_value_max returns.  PBVI_EUNSUPPORTED (-4) after an alpha-side backup
 * (pbvi_stats_t.formulation == 1).
 */
int pbvi_backup_fetch_value_max(pbvi_engine_t* e, double* out_value);
/* rows currently held by the stores (ids are 0 .. count-1) */
int64_t pbvi_belief_store_count(const pbvi_engine_t* e);
int64_t pbvi_alpha_store_count(const pbvi_engine_t* e);

/*
 * f32 engines re-score the candidates of every belief in fp64, so pbvi_value_max / pbvi_value_max_store return exact
 * maxima and first-maximum indices (np.argmax semantics).  compute_change only takes max|new - old| of the values and
 * compares it with eps * gamma / (1 - gamma) (src/pomdp.py:2167-2169, :2372): exact = 0 skips the re-scoring and
 * returns the fp32 GEMM's maxima (relative error ~1e-7, within the 1e-6 bar of fp32 engines); indices are then the
 * fp32 argmax.  Default 1.  No effect on f64 engines.
 * The setting covers those two calls only.  A backup with PBVI_BELIEF_DOMINANCE compares b.alpha'[b] > max_v b.alpha_v
 * strictly (src/pomdp.py:1510-1512): its maxima are re-scored in fp64 whatever this setting says, so the keep mask does
 * not depend on it (pbvi_debug_value_max_route reports route 2, or route 1, for that GEMM).
 */
int pbvi_set_value_max_exact(pbvi_engine_t* e, int exact);

/*
 * Batched belief update (Bayes step) of the resident belief block: the step that produces the beliefs the
 * backup consumes.  Replaces Belief.update (src/pomdp.py:382-421) applied to B beliefs at once (the
 * reference's own batched form lives in its simulator, src/pomdp.py:3277-3310):
 *   out[b] = normalise( sum_{s,r} b[b,s] * RTO[s, actions[b], observations[b], r]  scattered to rs[s,a,r] )
 *   actions, observations [B] int32 (caller's belief order); out_beliefs [B][S] T, host or device memory (pageable host
 *   memory through the pinned bounce buffer).
 * A belief whose update has zero mass (impossible observation) yields NaNs, as the reference's 0/0 does.
 */
int pbvi_belief_update(pbvi_engine_t* e, const int32_t* actions, const int32_t* observations, void* out_beliefs);

/*
 * Policy-evaluation step of the parallel simulator (Agent.run_n_simulations_parallel, src/pomdp.py:3296-3347)
 * on the resident belief block, which never leaves the device between steps:
 *   1. pbvi_value_max gives out_index[b] = first argmax_v b.alpha_v  (Agent.get_best_action, :3029); the caller
 *      maps it through ValueFunction.actions and runs its simulator (host RNG, SimulationSet.run_actions);
 *   2. pbvi_beliefs_advance replaces every belief by its Bayes update with (actions[b], observations[b])
 *      (:3306-3311) and drops the rows with keep[b] == 0 (:3326-3329, the done-filter); survivors keep the
 *      caller's order.  keep may be NULL (keep all).  *out_B (may be NULL) receives the new row count; when it
 *      is 0 no belief block is resident any more.
 * pbvi_beliefs_fetch copies the resident block out, [B][S] T in caller order (host or device memory; pageable host
 * memory through the pinned bounce buffer);
 * pbvi_beliefs_count returns B (0 = none, -1 = NULL handle).
 */
int pbvi_beliefs_advance(pbvi_engine_t* e, const int32_t* actions, const int32_t* observations, const uint8_t* keep,
                         int64_t* out_B);
int pbvi_beliefs_fetch(pbvi_engine_t* e, void* out_beliefs);
int64_t pbvi_beliefs_count(const pbvi_engine_t* e);

/*
 * Device-resident policy rollout: T lock-step steps of the parallel simulator (Agent.run_n_simulations_parallel,
 * src/pomdp.py:3203-3380, with SimulationSet.run_actions, :2893-2945, as its draw; the per-step loop of this package's host seam is the
 * pbvi_value_max / pbvi_q_values + host draw + pbvi_beliefs_advance chain above) for the resident belief block against the
 * resident alpha set, without leaving the device between steps.  Row b of the block is simulation first_sim_id + b.
 * For step t = 0 .. T-1 and every simulation i still running:
 *   action   lookahead 0: a = alpha_actions[first argmax_v b.alpha_v], decided as pbvi_value_max decides it;
 *            lookahead 1: a = first argmax_a Q(b, a), pbvi_q_values' out_action (discount gamma; unused for lookahead 0)
 *   uniform  u = uniform01(splitmix64(seed, i), t): x = seed + (idx + 1) * 0x9E3779B97F4A7C15; z = (x ^ x >> 30) *
 *            0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; hash = z ^ z >> 31 (all mod 2^64), applied to
 *            (seed, i) and then to (that hash, t); u = (hash >> 11) * 2^-53.  One uniform per simulation and step.
 *   draw     w[k] = (double) RTO[s, a, o, r], k = o * R + r, from the table the engine was created with (an fp32 engine's fp32
 *            values widened; never the pbvi_engine_set_rto_f64 copy); c[k] = c[k-1] + w[k] by sequential fp64 additions;
 *            k* = the first k with u * c[O*R-1] < c[k], or the last k with w[k] > 0 if rounding leaves none;
 *            o = k* / R, s' = reach_states[s, a, k* % R].  RTO[s,a,o,r] = P(r | s,a) P(o | s'_r, a), so this is the joint law
 *            of the reference's successor-then-observation draw (SimulationSet.run_actions, src/pomdp.py:2918-2932) from one uniform.
 *   belief   b <- update(b, a, o), as pbvi_beliefs_advance computes it
 *   done     end_mask[s'] != 0 finishes the simulation at step t: out_steps[i] = t + 1, it takes no further part
 *            (src/pomdp.py:3326-3329) and its later trajectory entries are -1.  Otherwise out_steps[i] = T.
 * A trajectory is a function of (model tables, alpha set, start belief, start state, seed, simulation id) alone: not of B,
 * of which other simulations share the block, or of how a large run is cut into calls (advance first_sim_id by the rows of
 * the earlier calls).
 *   alpha_actions [V] int32 (ValueFunction.actions), start_states [B] int32, end_mask [S] uint8 (non-zero = end state): host
 *   out_states [T+1][B] (row 0 = start_states), out_actions [T][B], out_observations [T][B], out_steps [B]: int32, host
 *   memory, caller's belief order; any of them may be NULL.  They arrive in one transfer at the end of the call.
 * Afterwards the resident block holds the beliefs of the simulations still running, in caller order (pbvi_beliefs_count /
 * pbvi_beliefs_fetch); when every simulation finished no block is resident, as after pbvi_beliefs_advance.  The alpha set
 * and both row stores are untouched; the backup's stage buffers are re-used (an earlier pbvi_backup_run's results can no
 * longer be fetched).  Every index array is validated on the host before the first launch.
 * PBVI_EINVAL: no resident belief block or alpha set, NULL input, a start state outside [0, S), an alpha_actions entry
 * outside [0, A), lookahead not 0 or 1, T < 1, or a model with a pair (s, a) whose RTO entries sum to 0 (nothing can follow
 * it).  PBVI_EUNSUPPORTED, with a pbvi_last_error text: lookahead 1 on a PBVI_DENSE engine (as pbvi_q_values), or
 * (T + 1) * B beyond the int32 trajectory slot index.  PBVI_ENOMEM as everywhere (pbvi_engine_after_oom): the trajectory
 * buffers, (3 T + 2) * B int32, are device memory of the engine and count against pbvi_debug_alloc_limit.
 */
int pbvi_rollout(pbvi_engine_t* e, const int32_t* alpha_actions /* [V] */, int lookahead, double gamma,
                 const int32_t* start_states /* [B] */, const uint8_t* end_mask /* [S] */, uint64_t first_sim_id, uint64_t seed,
                 int64_t T, int32_t* out_states /* [T+1][B] */, int32_t* out_actions /* [T][B] */,
                 int32_t* out_observations /* [T][B] */, int32_t* out_steps /* [B] */);

/*
 * Infotaxis: the expected entropy of the next belief, for every belief of the resident block and every action -- the greedy
 * information-gathering policy a solved olfactory-search policy is judged against.  No alpha set is needed or read.
 * For a belief row b, action a and observation o, over the table the engine was created with (an fp32 engine's fp32 values
 * widened to fp64; never the pbvi_engine_set_rto_f64 copy):
 *   u[s']   = sum over (s, r) with reach_states[s, a, r] == s' of (double) b[s] * (double) RTO[s, a, o, r], in fp64, entries in
 *             ascending s * R + r order (np.bincount's order; the sum pbvi_belief_update normalises)
 *   Z[a, o] = sum_s' u[s']                      ( = P(o | b, a) )
 *   N[a, o] = sum_s' u[s'] * ln u[s']            (terms with u[s'] == 0 add 0)
 *   G[b, a] = sum_o (Z * ln Z - N)              (terms with Z == 0 add 0; sequential over o)
 *           = sum_o P(o | b, a) * H(update(b, a, o)),  H the Shannon entropy in nats
 *   H[b]    = - sum_s b[s] * ln b[s]            (the entropy of the belief itself; terms with b[s] == 0 add 0)
 *   a*[b]   = the first a whose G[b, a] is strictly smaller than every earlier one; a NaN never wins and a row of NaNs gives 0:
 *             np.argmin(np.where(np.isnan(G), np.inf, G), axis=1).  It is taken from the row of out_g that is returned, so
 *             out_action[b] equals that argmin of out_g[b] exactly.
 * ln is the fp64 logarithm.  The sums over s' are taken in an order that differs from NumPy's but is fixed and uses no
 * atomics: a belief's results have the same bits from call to call, whatever other beliefs share the block and wherever
 * the belief stands in it.
 *   out_g [B][A] double (required); out_action [B] int32, out_p_obs [B][A][O] double ( = Z), out_entropy [B] double: may be
 *   NULL.  Host (or device) memory, caller's belief order.
 * The resident block, the alpha set and both row stores are untouched, and so are the backup's stage buffers.  Works on
 * PBVI_SPARSE and PBVI_DENSE engines and on both number formats: it needs what pbvi_belief_update needs.
 * PBVI_EINVAL: no resident belief block, or out_g == NULL.  PBVI_ENOMEM as everywhere (pbvi_engine_after_oom): the partial
 * sums, ceil(S / 2048) * B * A * O * 2 doubles, and the results are device memory of the engine and count against
 * pbvi_debug_alloc_limit.
 */
int pbvi_infotaxis(pbvi_engine_t* e, double* out_g /* [B][A], required */, int32_t* out_action /* [B], may be NULL */,
                   double* out_p_obs /* [B][A][O], may be NULL */, double* out_entropy /* [B], may be NULL */);

/*
 * HSVI upper bound: the sawtooth interpolation over (belief, value) points above the corner values
 * (BeliefValueMapping.evaluate, src/pomdp.py:873-895), with the minimum restricted to the support of the point -- the
 * reference divides over all states and returns NaN (0/0) for every belief that shares a zero with a point, which is every
 * belief of a sparse model.  Where the reference's expression is finite the two agree.
 * The point store: one per engine, append-only with a reset, rows kept sparse (CSR: int32 state, fp64 value) in device
 * memory of the engine (counted against pbvi_debug_alloc_limit, PBVI_ENOMEM as everywhere; released by
 * pbvi_engine_after_oom, after which the store is empty and no corner is set).
 *   pbvi_upper_reset   empties the store and sets the corner values c [S] fp64 (finite).
 *   pbvi_upper_append  n points behind the ones held: points [n][S] fp64 (entries finite and >= 0, not all zero), values [n]
 *                      = v_i, gaps [n] = gap_i = v_i - p_i . c, computed ONCE by the caller so that host and device hold the
 *                      same bits.  PBVI_EINVAL: no corner set, NULL, a bad entry, a NaN value or gap.
 *   pbvi_upper_count   points held (-1: NULL handle).
 * For a belief row b (an fp32 engine's rows widened to fp64) and points i:
 *   v0     = sum_s b[s] * c[s]
 *   r_i    = min over s with p_i[s] > 0 of b[s] / p_i[s]        (IEEE fp64 division; the minimum is exact, so order-free)
 *   w_i    = v0 + gap_i * r_i                                    (one rounded multiply, one rounded add, never fused)
 *   U(b)   = min(v0, min_{i < n_visible} w_i);   point = the first i attaining it, -1 when v0 <= every w_i
 *   hit(b) = the first i < n_hit with p_i[s] == b[s] for every s, else -1   (equality on the support of p_i and
 *            nnz(b) == nnz(p_i), which together are exact)
 *   value  = v_hit if hit >= 0 (the reference's dictionary shortcut, :884), else U(b)
 * A row that holds a NaN gives value NaN, point -1, hit -1.  n_visible <= n_hit <= count restate the reference's stale
 * cache: its stacked arrays see the points of the last update(), its dictionary every add at once.
 * v0 is summed in a fixed order that differs from NumPy's; nothing is accumulated with atomics: a belief's results have the
 * same bits from call to call, whatever other beliefs share the block and wherever the belief stands in it.
 *
 * pbvi_upper_bound: the above for every belief of the resident block.  out_value [B] double (required); out_point [B],
 * out_hit [B] int32 may be NULL.  Host (or device) memory, caller's belief order.
 *
 * pbvi_upper_q: the action values the HSVI descent is greedy for (expand_hsvi, src/pomdp.py:1768-1868), over the table the
 * engine was created with (fp32 values widened; never the pbvi_engine_set_rto_f64 copy):
 *   u[s']     = pbvi_infotaxis' sum;   Z[a, o] = sum_s' u[s'], the 256-state blocks' sums added in block order (the
 *               fixed-order normaliser of pbvi_rollout_infotaxis, not the atomic one: the hit test needs successor bits that
 *               repeat);   b_ao = (T)(u / Z), the successor as pbvi_belief_update rounds it
 *   Q[b, a]   = sum_s b[s] * ER[s, a] + gamma * sum_o Z[a, o] * value(b_ao)      (sequential over o; Z == 0 adds 0)
 *   a*[b]     = the first maximum of the row of out_q that is returned; a NaN never wins and a row of NaNs gives 0
 *   out_q [B][A] double (required); out_action [B] int32, out_p_obs [B][A][O] double ( = Z), out_succ_value [B][A][O] double
 *   ( = value(b_ao), NaN where Z == 0): may be NULL.  Caller's belief order.
 * The successors are materialised in chunks of beliefs sized to half the memory the engine may still take (one belief at
 * the least): (sizeof(double) + sizeof(T)) * S bytes per (belief, action, observation).
 *
 * Both calls leave the resident block, the alpha set, both row stores and the backup's stage buffers untouched (an earlier
 * pbvi_backup_run's results can still be fetched), and work on PBVI_SPARSE and PBVI_DENSE engines and both number formats.
 * PBVI_EINVAL: a NULL required output, no resident belief block, no corner set, n_visible > n_hit, n_hit > count.
 * PBVI_EUNSUPPORTED (pbvi_upper_q): A * O > 65535.  PBVI_ENOMEM as everywhere (pbvi_engine_after_oom).
 */
int pbvi_upper_reset(pbvi_engine_t* e, const double* corner /* [S] */);
int pbvi_upper_append(pbvi_engine_t* e, const double* points /* [n][S] */, const double* values /* [n] */,
                      const double* gaps /* [n] */, int64_t n);
int64_t pbvi_upper_count(const pbvi_engine_t* e);
int pbvi_upper_bound(pbvi_engine_t* e, int64_t n_visible, int64_t n_hit, double* out_value /* [B], required */,
                     int32_t* out_point /* [B], may be NULL */, int32_t* out_hit /* [B], may be NULL */);
int pbvi_upper_q(pbvi_engine_t* e, double gamma, int64_t n_visible, int64_t n_hit, double* out_q /* [B][A], required */,
                 int32_t* out_action /* [B], may be NULL */, double* out_p_obs /* [B][A][O], may be NULL */,
                 double* out_succ_value /* [B][A][O], may be NULL */);

/*
 * Device-resident infotaxis rollout: pbvi_rollout with the action of every step taken from pbvi_infotaxis' a*[b] instead of
 * the alpha set -- a = the first argmin_a G(b, a) of the simulation's current belief.  Everything else is pbvi_rollout's:
 * the uniform u(i, t) = uniform01(splitmix64(seed, i), t) of simulation i = first_sim_id + b, the (o, s') draw from
 * RTO[s, a, :, :] by sequential fp64 prefix sums, the done rule (end_mask[s'] != 0 finishes the simulation at step t:
 * out_steps[i] = t + 1, later entries -1, otherwise out_steps[i] = T), the Bayes step, the dropping of finished rows after
 * every step, the layout of the trajectory buffers (out_states [T+1][B] with row 0 = start_states, out_actions [T][B],
 * out_observations [T][B], out_steps [B], int32, caller order, any may be NULL) and the end state of the block (the
 * beliefs of the simulations still running, in caller order; none resident when all finished).  No alpha set is needed.
 * One difference in arithmetic: the Bayes step of this call adds a belief's per-block masses in block order instead of with
 * atomic adds (the last bit of the normaliser then does not depend on arrival order), because infotaxis meets near-ties
 * between actions: a trajectory is a function of (model tables, start belief, start state, seed, simulation id) alone.
 * PBVI_EINVAL: no resident belief block, NULL start_states or end_mask, a start state outside [0, S), T < 1, or a model with
 * a pair (s, a) whose RTO entries sum to 0.  PBVI_EUNSUPPORTED: (T + 1) * B beyond the int32 trajectory slot index.
 * PBVI_ENOMEM as everywhere.
 */
int pbvi_rollout_infotaxis(pbvi_engine_t* e, const int32_t* start_states /* [B] */, const uint8_t* end_mask /* [S] */,
                           uint64_t first_sim_id, uint64_t seed, int64_t T, int32_t* out_states /* [T+1][B] */,
                           int32_t* out_actions /* [T][B] */, int32_t* out_observations /* [T][B] */,
                           int32_t* out_steps /* [B] */);

/*
 * Environments: where the observations of pbvi_rollout_env come from.  The rollouts above simulate the world the agent
 * believes in (successor and observation both from the engine's RTO); an evaluation against recorded data or a mismatched
 * sensor replaces the observation source and keeps the agent's model for the Bayes step.  One environment per engine, held
 * in device memory of the engine (counted against pbvi_debug_alloc_limit, PBVI_ENOMEM as everywhere; released by
 * pbvi_engine_after_oom, after which no environment is set).  Setting one kind replaces the other.
 *   pbvi_env_set_frames  frames [F][C][S] uint8: frames[f][c][s] = the observation id emitted in frame f, channel c, at state s;
 *                        channel_of_action [A] int32: the channel an action reads (nose / ground data: C = 2).
 *                        PBVI_EINVAL: NULL, F or C < 1, a channel outside [0, C), a frame entry >= O.
 *                        PBVI_EUNSUPPORTED: O > 255 (one byte per entry).
 *   pbvi_env_set_table   obs_prob [S][A][O] double: obs_prob[s', a, :] = the law of the observation after landing in s' with
 *                        action a (need not be normalised).  PBVI_EINVAL: NULL, an entry negative or not finite, a row that
 *                        sums to 0.
 *   pbvi_env_clear       no environment; the bytes are returned.
 * All three validate on the host, leave a pbvi_last_error text, and do not touch the belief block, the alpha set or the stores.
 */
int pbvi_env_set_frames(pbvi_engine_t* e, const uint8_t* frames /* [F][C][S] */, int64_t F, int64_t C,
                        const int32_t* channel_of_action /* [A] */);
int pbvi_env_set_table(pbvi_engine_t* e, const double* obs_prob /* [S][A][O] */);
int pbvi_env_clear(pbvi_engine_t* e);

/*
 * Device-resident rollout against the environment: pbvi_rollout's loop, trajectory layout (-1 padding included) and end state of
 * the block, with the policy chosen by number and the observation taken from the environment.
 *   policy   0: a = alpha_actions[first argmax_v b.alpha_v];  1: a = first argmax_a Q(b, a) (discount gamma; PBVI_SPARSE
 *            engines);  2: infotaxis, a = first argmin_a G(b, a) (alpha_actions may be NULL, no alpha set needed)
 * For simulation i = first_sim_id + b at step t, in state s, with that action a:
 *   successor    w[r] = sum_o (double) RTO[s, a, o, r], o ascending, sequential fp64 adds ( = P(r | s, a) from the table the
 *                engine scores with);  c[r] = c[r-1] + w[r];  r* = the first r with u1 * c[R-1] < c[r], else the last r with
 *                w[r] > 0;  u1 = uniform01(splitmix64(seed, i), t), pbvi_rollout's uniform;  s' = reach_states[s, a, r*].
 *                A model with a pair (s, a) whose RTO entries sum to 0 is refused, as by pbvi_rollout.
 *   observation  o = end_observation                               if end_observation >= 0 and end_mask[s'];
 *                o = frames[shift_i + t][channel_of_action[a]][s']   with a frame environment (shift_i = shifts[b], 0 if NULL);
 *                o drawn from obs_prob[s', a, :] by the same sequential-prefix rule with a second uniform
 *                  u2 = uniform01(splitmix64(seed, i), 2^32 + t)   with a table environment (t < 2^31: the streams never meet)
 *   done         end_mask[s'] != 0 finishes the simulation: out_steps[i] = t + 1, out_lost[i] = 0, no belief update
 *   lost         otherwise, with u the un-normalised Bayes step of (b, a, o) and Z = sum_s' u[s']: if Z == 0 or Z is not finite,
 *                the observation was impossible under the agent's model and the simulation stops at this step:
 *                out_steps[i] = t + 1, out_lost[i] = 1.  Its step-t action, observation and s' are recorded, its row is
 *                dropped like a finished one, and no NaN belief is ever formed.  Z is a sum of non-negative products, so
 *                Z == 0 does not depend on the order of the sum.
 *   belief       otherwise b <- u / Z, with Z summed in block order (no atomics) for every policy
 * A trajectory is a function of (model tables, alpha set, environment, start belief, start state, shift, seed, id) alone: not
 * of B, of the other simulations in the block, or of how a run is cut into calls.
 *   shifts [B] int64 or NULL (frames only); out_lost [B] uint8, may be NULL; the rest as pbvi_rollout.
 * Every check is made on the host before the first launch.  PBVI_EINVAL beyond pbvi_rollout's: no environment set, policy not
 * 0, 1 or 2, end_observation >= O, shifts given with a table environment, a negative shift, or max(shift) + T > F (the
 * reference would index past its data).  PBVI_ENOMEM as everywhere.
 */
int pbvi_rollout_env(pbvi_engine_t* e, int policy, const int32_t* alpha_actions /* [V] */, double gamma,
                     const int32_t* start_states /* [B] */, const uint8_t* end_mask /* [S] */, int end_observation,
                     const int64_t* shifts /* [B] or NULL */, uint64_t first_sim_id, uint64_t seed, int64_t T,
                     int32_t* out_states /* [T+1][B] */, int32_t* out_actions /* [T][B] */,
                     int32_t* out_observations /* [T][B] */, int32_t* out_steps /* [B] */, uint8_t* out_lost /* [B] */);

/*
 * Space-aware infotaxis (Loisy & Eloy 2022): the greedy policy for J(b) = log2(D(b) + 2^(H(b) - 1) - 1/2), D the expected
 * distance to the source and H the entropy in bits -- the baseline the olfactory-search literature judges solved policies
 * against.  The distance enters as one vector of state weights, so the same call gives a second baseline, the expected
 * weight of the successor ("greedy distance" with a distance, a QMDP-style policy with w = -V_MDP shifted to >= 0).
 *
 * State weights: one vector per engine, w [S] fp64, every entry finite and >= 0 (checked on the host).
 *   pbvi_state_weights_set    sets it (PBVI_EINVAL with a pbvi_last_error text: NULL, or an entry negative or not finite).
 *   pbvi_state_weights_clear  removes it; the bytes are returned.
 * The vector is device memory of the engine, S doubles exactly, counted against pbvi_debug_alloc_limit (PBVI_ENOMEM as
 * everywhere) and released by pbvi_engine_after_oom, after which no weights are set.  Setting or clearing weights touches
 * nothing else: not the belief block, the alpha set, the stores, the environment or any result.
 *
 * For a belief row b, action a and observation o, u[s'], Z[a, o] and N[a, o] are exactly pbvi_infotaxis' (the table the
 * engine was created with, an fp32 engine's values widened to fp64; never the pbvi_engine_set_rto_f64 copy), and
 *   D[a, o] = sum_s' u[s'] * w[s']                  (terms with u[s'] == 0 add 0)
 * Per (a, o) with Z != 0:
 *   H = max(0, ln Z - N / Z)                        the entropy of the successor belief, in nats
 *   d = D / Z                                       its expected weight
 *   x = max(1, d + (exp(H) - 1) / 2)                ( = d + 2^(H_bits - 1) - 1/2 )
 *   J = log2(x)
 * Both clamps are part of the definition (max as C's fmax).  Rounding can make ln Z - N / Z slightly negative: the first
 * removes that.  The second gives J >= 0: a successor known to sit on the source (H = 0, d = 0) gives J = 0, the paper's
 * value for "found".  Neither -inf nor NaN can arise from finite inputs.
 *   objective 0 (space-aware):     F[b, a] = sum_o Z * J
 *   objective 1 (expected weight): F[b, a] = sum_o D
 * Both sums run sequentially over o; an observation with Z == 0 adds 0.
 *   a*[b] = the first a whose F[b, a] is strictly below every earlier one; a NaN never wins and a row of NaNs gives 0.  It is
 *           taken from the row of out_f that is returned, so out_action[b] equals that argmin of out_f[b] exactly.
 * ln, exp and log2 are the fp64 functions.  The sums over s' are taken in pbvi_infotaxis' order -- fixed, no atomics: a
 * belief's results have the same bits from call to call, whatever other beliefs share the block and wherever it stands.
 *
 * pbvi_space_aware: the above for every belief of the resident block.
 *   out_f [B][A] double (required); out_action [B] int32, out_terms [B][A][O][3] double = (Z, N, D): may be NULL.  Host (or
 *   device) memory, caller's belief order.
 * The resident block, the alpha set, both row stores, the backup's stage buffers and pbvi_infotaxis' results are untouched.
 * Works on PBVI_SPARSE and PBVI_DENSE engines and on both number formats.
 * PBVI_EINVAL: no resident belief block, no weights set, out_f == NULL, or an objective other than 0 or 1.  PBVI_ENOMEM as
 * everywhere (pbvi_engine_after_oom): the partial sums, ceil(S / 2048) * B * A * O * 3 doubles, and the results are device
 * memory of the engine and count against pbvi_debug_alloc_limit.
 *
 * pbvi_rollout_space_aware: the step loop of the rollouts above with a fourth action source, a = a*[b] of the simulation's
 * current belief under `objective`.
 *   use_env = 0  the model's world, as pbvi_rollout_infotaxis: draws, done rule, trajectory layout and end state of the
 *                block are pbvi_rollout's.  end_observation must be -1 and shifts NULL; out_lost, if given, is all 0.
 *   use_env = 1  the successor draw, observation source, lost rule and checks of pbvi_rollout_env, against the environment
 *                set with pbvi_env_set_*.
 * In both cases the Bayes step's mass is summed in block order, with no atomics, as for infotaxis: a trajectory is a function
 * of (model tables, weights, objective, environment, start belief, start state, shift, seed, id) alone.  No alpha set is
 * needed.  PBVI_EINVAL beyond those of pbvi_rollout_infotaxis / pbvi_rollout_env: no weights set, an objective other than 0 or
 * 1, use_env other than 0 or 1, end_observation or shifts given with use_env = 0.  pbvi_rollout_env itself keeps refusing
 * policy numbers other than 0, 1 and 2: this source is reachable through this entry point only.
 */
int pbvi_state_weights_set(pbvi_engine_t* e, const double* weights /* [S] */);
int pbvi_state_weights_clear(pbvi_engine_t* e);
int pbvi_space_aware(pbvi_engine_t* e, int objective, double* out_f /* [B][A], required */,
                     int32_t* out_action /* [B], may be NULL */, double* out_terms /* [B][A][O][3], may be NULL */);
int pbvi_rollout_space_aware(pbvi_engine_t* e, int objective, int use_env, const int32_t* start_states /* [B] */,
                             const uint8_t* end_mask /* [S] */, int end_observation, const int64_t* shifts /* [B] or NULL */,
                             uint64_t first_sim_id, uint64_t seed, int64_t T, int32_t* out_states /* [T+1][B] */,
                             int32_t* out_actions /* [T][B] */, int32_t* out_observations /* [T][B] */,
                             int32_t* out_steps /* [B] */, uint8_t* out_lost /* [B] */);

/*
 * State policies: the three heuristics that act through a policy of the underlying MDP, pi(s), instead of value rows --
 * most likely state, action voting (Cassandra's MDP heuristics; "most likely state" and "voting" of Loisy & Eloy 2022) and
 * Thompson / posterior sampling.  One reduction over S per belief, no GEMM.
 *
 * State policy table: one per engine, state_actions [S] int32, every entry in [0, A) (checked on the host).
 *   pbvi_state_policy_set    sets it (PBVI_EINVAL with a pbvi_last_error text: NULL, or an entry outside [0, A)).
 *   pbvi_state_policy_clear  removes it; the bytes are returned.
 * The table is device memory of the engine, S int32 exactly, counted against pbvi_debug_alloc_limit (PBVI_ENOMEM as
 * everywhere) and released by pbvi_engine_after_oom, after which no table is set.  Setting or clearing it touches nothing
 * else: not the belief block, the alpha set, the stores, the weights, the environment or any result.
 *
 * A belief row b is the resident row widened to fp64 (an fp32 engine's values are widened, exactly as pbvi_infotaxis reads
 * them).  Chunk c is the states [256 c, min(256 c + 256, S)), C = ceil(S / 256).  Every sum below is taken by sequential fp64
 * adds in the order stated, starting from +0.0 -- fixed, no atomics: a belief's results have the same bits from call to call,
 * whatever other beliefs share the block and wherever it stands, and equal pomdp.state_policy_numpy's bit for bit.
 *   rule 0 (most likely state)
 *     s* = the first s whose b[s] is strictly greater than every earlier entry (a NaN never wins; a row of NaNs gives 0)
 *     a = state_actions[s*];  out_state = s*
 *   rule 1 (voting)
 *     W_c[a] = sum over the states s of chunk c, ascending, of b[s] where state_actions[s] == a (other states add nothing)
 *     W[a]   = W_0[a] + W_1[a] + ... in chunk order
 *     a* = the first a whose W[a] is strictly greater than every earlier one, taken from the row of out_votes that is
 *          returned;  out_state = -1
 *   rule 2 (Thompson)
 *     u       the uniform of the belief: uniforms[b] when uniforms is given, else uniform01(splitmix64(seed, i), 2^33 + t) with
 *             i = first_sim_id + b -- a third counter stream beside the rollouts' t and 2^32 + t (t < 2^31 keeps them apart)
 *     q_c[j]  the sequential prefix sums of b inside chunk c;  m_c = q_c[last];  P_c = P_{c-1} + m_c;  total = P_{C-1}
 *     target = u * total (one rounded multiply)
 *     c* = the first c with target < P_c; if there is none, the last c with m_c > 0
 *     r  = target - (c* > 0 ? P_{c*-1} : 0) (one rounded subtract)
 *     s~ = the first state j of chunk c* with r < q_{c*}[j]; if there is none, the last state of that chunk with b > 0
 *     a = state_actions[s~];  out_state = s~.  The drawn state always has b[s~] > 0.  (A row without any mass, which is no
 *     belief, gives c* = 0 and s~ = 0.)
 *
 * pbvi_state_policy: the above for every belief of the resident block.
 *   out_action [B] int32 (required); out_state [B] int32, out_votes [B][A] double (written by rule 1 only): may be NULL.
 *   uniforms [B] double or NULL (rule 2 only); every entry in [0, 1] -- 1.0 itself is accepted: it is the only way to reach
 *   the two fallbacks on purpose.  Host (or device) memory, caller's belief order.
 * The resident block, the alpha set, both row stores, the backup's stage buffers and the other greedy policies' results are
 * untouched.  Works on PBVI_SPARSE and PBVI_DENSE engines and on both number formats.
 * PBVI_EINVAL: no resident belief block, no table set, a rule other than 0, 1 or 2, out_action == NULL, a uniforms entry
 * outside [0, 1] (or NaN), uniforms given for a rule other than 2, t < 0 or t >= 2^31.  PBVI_ENOMEM as everywhere
 * (pbvi_engine_after_oom): the results and rule 2's per-chunk sums, B * C * 2 doubles, are device memory of the engine and
 * count against pbvi_debug_alloc_limit.
 *
 * pbvi_rollout_state_policy: the step loop of the rollouts above with a fifth action source, the action of `rule` for the
 * simulation's current belief; Thompson's uniform of simulation i at step t is uniform01(splitmix64(seed, i), 2^33 + t).
 * use_env, the Bayes step's mass in block order, the trajectory layout, the end state of the block and the checks are
 * pbvi_rollout_space_aware's, with "no state policy set" and the rule in place of the weights and the objective.  No alpha
 * set is needed.  pbvi_rollout_env itself keeps refusing policy numbers other than 0, 1 and 2.
 */
int pbvi_state_policy_set(pbvi_engine_t* e, const int32_t* state_actions /* [S] */);
int pbvi_state_policy_clear(pbvi_engine_t* e);
int pbvi_state_policy(pbvi_engine_t* e, int rule, uint64_t seed, uint64_t first_sim_id, int64_t t,
                      const double* uniforms /* [B] or NULL */, int32_t* out_action /* [B], required */,
                      int32_t* out_state /* [B], may be NULL */, double* out_votes /* [B][A], may be NULL */);
int pbvi_rollout_state_policy(pbvi_engine_t* e, int rule, int use_env, const int32_t* start_states /* [B] */,
                              const uint8_t* end_mask /* [S] */, int end_observation, const int64_t* shifts /* [B] or NULL */,
                              uint64_t first_sim_id, uint64_t seed, int64_t T, int32_t* out_states /* [T+1][B] */,
                              int32_t* out_actions /* [T][B] */, int32_t* out_observations /* [T][B] */,
                              int32_t* out_steps /* [B] */, uint8_t* out_lost /* [B] */);

/*
 * MDP value iteration on the device (VI_Solver.solve, src/mdp.py:1442-1525; seeds FSVI / HSVI):
 *   rows[a][s] = ER[s,a] + gamma * sum_r P[s,a,r] * v[rs[s,a,r]];   v'[s] = max_a rows[a][s]
 * repeated from v0 until max_s |v' - v| < max_change_limit (the reference's eps * gamma / (1 - gamma)) or
 * `horizon` sweeps.  Always fp64.  Not tied to an engine handle (the MDP tables are not the POMDP's).
 *   reach_states [S][A][R] int32, reach_prob [S][A][R], exp_reward [S][A], v0 [S]   (NumPy C-order)
 *   out_rows [A][S]: rows of the last sweep (the solution's alpha-vectors, before the container's dedup); all 0.0 for
 *   horizon = 0 (PBVI_OK, zero iterations)
 *   out_changes [horizon] (may be NULL): max change of each sweep that ran;  out_iterations (may be NULL).
 * The three handle-free sweep entries (this one, pbvi_fib_value_iteration, pbvi_controller_value_iteration) share one run
 * driver (csrc/engine.hip, SweepRun) and one kernel file (csrc/sweep_kernels.hip).
 */
int pbvi_mdp_value_iteration(int device, int32_t S, int32_t A, int32_t R, const int32_t* reach_states,
                             const double* reach_prob, const double* exp_reward, const double* v0, double gamma,
                             double max_change_limit, int32_t horizon, double* out_rows, double* out_changes,
                             int32_t* out_iterations);

/*
 * Fast Informed Bound on the device (Hauskrecht 2000; FIB_Solver.solve, the initial upper bound of HSVI with
 * upper_init='fib'): the MDP sweep with the observation kept inside the maximisation,
 *   Q'[s][a] = ER[s,a] + gamma * sum_o max_a' sum_r RTO[s,a,o,r] * Q[rs[s,a,r]][a']
 * repeated from q0 until max_{s,a} |Q' - Q| < max_change_limit (eps * gamma / (1 - gamma)) or `horizon` sweeps.  From the
 * same start it is never above the MDP rows (sum_o RTO = P) and still an upper bound of the POMDP value; with one
 * successor per (s, a) it equals them.  Always fp64.  Not tied to an engine handle.
 * One sweep, operation for operation (products and sums un-fused; pomdp.fib_numpy is the same statement in NumPy, and
 * rows and changes agree with it bit for bit on finite inputs):
 *   for o = 0..O-1:  acc[a'] = RTO[s,a,o,0] * Q[rs[s,a,0]][a'], then acc[a'] += RTO[s,a,o,r] * Q[rs[s,a,r]][a'], r = 1..R-1;
 *                    m_o = max_a' acc[a'];   tot = m_0, then tot += m_o in order;
 *   Q'[s][a] = ER[s,a] + gamma * tot.
 *   reach_states [S][A][R] int32, rto [S][A][O][R], exp_reward [S][A], q0 [A][S]   (NumPy C-order)
 *   out_rows [A][S]: the rows of the last sweep that ran (A action-labelled alpha-vectors); q0 itself for horizon = 0
 *   out_changes [horizon] (may be NULL): max change of each sweep that ran;  out_iterations (may be NULL).
 * PBVI_EINVAL (bad sizes, NULL tables, a negative horizon, a reachable state outside [0, S)) and PBVI_EUNSUPPORTED
 * (S*A*O*R beyond int32) are decided before the device is touched.
 */
int pbvi_fib_value_iteration(int device, int32_t S, int32_t A, int32_t O, int32_t R, const int32_t* reach_states,
                             const double* rto, const double* exp_reward, const double* q0, double gamma,
                             double max_change_limit, int32_t horizon, double* out_rows, double* out_changes,
                             int32_t* out_iterations);

/*
 * Exact value of a finite-state controller (policy graph) on the device; the blind-policy lower bound (Hauskrecht 1997;
 * Blind_Solver.solve, the initial lower bound of HSVI with lower_init='blind') is the controller with N = A, a_n = n,
 * succ[n][o] = n.  Node n takes action a_n = node_action[n] and moves to node succ[n][o] = node_succ[n][o] on observation o:
 *   V'[n][s] = ER[s,a_n] + gamma * sum_o sum_r RTO[s,a_n,o,r] * V[succ[n][o]][rs[s,a_n,r]]
 * as Jacobi sweeps (all of V' from the old V), repeated from v0 until max_{n,s} |V' - V| < max_change_limit
 * (eps * gamma / (1 - gamma)) or `horizon` sweeps.  Every row of the fixed point is the value of a policy that can be run
 * under partial observability, so the rows are valid alpha-vectors (a lower bound of the POMDP value); from a start below
 * the fixed point (min ER / (1 - gamma)) the iterates rise towards it and a run stopped anywhere is still below it.  Always
 * fp64.  Not tied to an engine handle.
 * One sweep, operation for operation (products and sums un-fused; pomdp.controller_numpy is the same statement in NumPy,
 * and rows and changes agree with it bit for bit on finite inputs), with a = a_n:
 *   for o = 0..O-1:  acc_o = RTO[s,a,o,0] * V[succ[n][o]][rs[s,a,0]], then acc_o += RTO[s,a,o,r] * V[succ[n][o]][rs[s,a,r]],
 *                    r = 1..R-1;   tot = acc_0, then tot += acc_o in order;
 *   V'[n][s] = ER[s,a] + gamma * tot.
 *   reach_states [S][A][R] int32, rto [S][A][O][R], exp_reward [S][A], node_action [N] int32, node_succ [N][O] int32,
 *   v0 [N][S]   (NumPy C-order)
 *   out_rows [N][S]: the rows of the last sweep that ran, row n the value of starting in node n; v0 itself for horizon = 0
 *   out_changes [horizon] (may be NULL): max change of each sweep that ran;  out_iterations (may be NULL).
 * PBVI_EINVAL (bad sizes, NULL tables, a negative horizon, a reachable state outside [0, S), a node action outside [0, A), a
 * successor outside [0, N)) and PBVI_EUNSUPPORTED (S*A*O*R or N*ceil(S/256) beyond int32; sizes alone decide it, before any
 * table is read) are decided before the device is touched.  PBVI_ENOMEM when the device has no room; a call leaves no
 * device memory behind.
 */
int pbvi_controller_value_iteration(int device, int32_t S, int32_t A, int32_t O, int32_t R, const int32_t* reach_states,
                                    const double* rto, const double* exp_reward, int32_t N, const int32_t* node_action,
                                    const int32_t* node_succ, const double* v0, double gamma, double max_change_limit,
                                    int32_t horizon, double* out_rows, double* out_changes, int32_t* out_iterations);

/*
 * Belief walk of the FSVI-style expansions (PBVI_Solver.expand_fsvi / expand_fsvi_eg, src/pomdp.py:1895-1935; the
 * trajectory of (action, observation) pairs is simulated by the caller in the underlying MDP and does not depend
 * on the beliefs): n chained Bayes updates (Belief.update, :382-421) entirely on the device, in fp64,
 *   b_{i+1} = update(restart[i] ? b0 : b_i, actions[i], observations[i]),        b_0 = b0
 * Each b_{i+1} is appended to the belief row store (so the following backup selects it by id with no upload) and
 * copied to out_beliefs [n][S] fp64 (host), which the caller's containers need for their byte-keyed dedup.
 * restart may be NULL (never).  Returns the store id of b_1 (b_{i+1} has id + i), or a negative error code.
 */
int64_t pbvi_belief_walk(pbvi_engine_t* e, const double* b0, int64_t n, const int32_t* actions, const int32_t* observations,
                         const uint8_t* restart, double* out_beliefs);
/*
 * Dedup keys of the n beliefs of the last pbvi_belief_walk: out_keys[i] = sum_s bits(row i, s) * (2 s + 1) mod 2^64 over
 * the 64-bit patterns of the fp64 row i (the hash of pbvi_backup_fetch_row_hashes) -- the integer the host's belief containers hash on in place of the row's bytes (BeliefSet.union,
 * src/pomdp.py:585-606, keys its dictionaries on values.tobytes()) -- so the host does not pass over the rows again.
 */
int pbvi_belief_walk_keys(pbvi_engine_t* e, int64_t n, uint64_t* out_keys);
/* Optional fp64 copy of RTO ([S][A][O][R], as at creation) for pbvi_belief_walk on an f32 engine, so the fp64 belief
 * values it returns do not depend on the engine's arithmetic type (f64 engines read their own table). */
int pbvi_engine_set_rto_f64(pbvi_engine_t* e, const double* rto);

/*
 * Which operand of the score GEMM is projected through the model (sparse mode; same scores, re-associated):
 *   1 = alpha-vectors, the reference's order (Gamma[a,o,v,:], src/pomdp.py:1489-1491; GEMM [B] x [A*O*V]);
 *   2 = beliefs (bp[a,o,b,:] = gamma * sum b[s] RTO[s,a,o,r] scattered to rs[s,a,r]; GEMM [B*A*O] x [V]);
 *   0 = automatic (default): the cheaper of the two by projected rows and 256-row tile count -- the belief side
 *       when B << V, e.g. the solve loop's ~100 new beliefs against thousands of alpha-vectors -- unless Gamma and its
 *       score slabs exceed what the engine may still allocate (its cap, or the free device memory) while the projected
 *       beliefs fit: then the belief side, whatever it costs.  (The reference dies there: Sea_Robin_Real.ipynb:913.)
 */
int pbvi_set_formulation(pbvi_engine_t* e, int formulation);

/*
 * fp64 engines only (a no-op setting on fp32 ones): the fp32 SCREEN.  mode 1 (default): when the score GEMM is large
 * the scores are computed by the fp32 stream-K GEMM on fp32-rounded copies of the operands, with the tie window widened
 * by the input roundings, and every (belief, action, observation) and action whose winner is not clear is re-decided
 * from the fp64 originals -- same indices and values as the pure fp64 pipeline up to that pipeline's own summation
 * order, at about the fp32 engine's speed (the fp64 MFMA GEMM sustains a third of the fp32 one).  0: never (pure
 * fp64 arithmetic throughout, src/pomdp.py:1485-1506 literally); 2: always, whatever the size (tests).
 * PBVI_F64_SCREEN=off|auto|always in the environment sets the initial mode.
 */
int pbvi_set_f64_screen(pbvi_engine_t* e, int mode);

/*
 * fp32 scoring with one reachable state per (s, a) (every large model of the reference): 1 (default) = the score GEMM
 * generates the Gamma tiles (src/pomdp.py:1485-1491) on the way into LDS instead of reading a projected copy from HBM;
 * 0 = project first (k_project), then multiply -- the same scores bit for bit, kept for A/B measurements.
 * 2 = also with 2..7 reachable states per (s, a) (the padded-ELL SpMM inside the operand staging; bit-identical again, but
 * measured SLOWER than projecting first at |S| = 30000, R = 5 -- five shifted alpha windows per K step cost more L2 /
 * Infinity-Cache traffic than reading the projected tile once -- so it is never chosen automatically).  No effect where
 * the fused path does not apply (R > 7, successor maps without grid structure, fp64 scoring, belief-side formulation,
 * dense mode).
 */
int pbvi_set_fused_projection(pbvi_engine_t* e, int enable);

/*
 * fp32 engines (a no-op setting on fp64 ones and on their fp32 screen): where the backup's alpha-side score GEMM runs.
 * 1 (default) = on bf16 MFMAs with a three-term operand split (x = hi + lo, products hi*hi + hi*lo + lo*hi, fp32
 * accumulation) when the GEMM is large, with the near-tie window widened by the split's error bound, so indices,
 * actions and alpha' rows are those of the fp32 GEMM; 0 = never; 2 = always (tests).  The fp32 GEMM is kept for the
 * value-max GEMMs, the belief-side formulation and after pbvi_set_tie_window(rel > 0).  With R > 1 reachable states
 * per (s, a) the split reads the projected Gamma rows: pbvi_set_fused_projection(2) then does not fuse.
 * PBVI_SCORE_SPLIT=off|auto|always in the environment sets the initial mode.  pbvi_stats_t.score_split reports it.
 */
int pbvi_set_score_split(pbvi_engine_t* e, int mode);

/*
 * Gamma tiled over the alpha set (alpha-side formulation, sparse mode, engines that hold the projected rows in HBM: R > 1,
 * fp64 scoring and its fp32 screen, R = 1 after pbvi_set_fused_projection(0)).  The alpha set is walked in chunks of
 * chunk_rows rows: each chunk is projected into one chunk-sized Gamma buffer, multiplied, and its split-K partial slabs are
 * folded (in the slab order the argmax uses) into a full-width score matrix [B][A*O*(V+1)+2A]; argmax, refinement, action
 * stage, dedup and assembly then run once on that matrix, so first-max ties go to the lowest GLOBAL alpha index and the
 * results are those of the untiled call.  The refinement's level-1 screen (it reads the projected rows) is off in a
 * tiled call; the tie window is the widest over the chunks' GEMM plans.
 *   mode 0 (default): never -- Gamma is held whole;  1: automatic -- only when Gamma and its score slabs do not fit what
 *   the engine may still allocate (then, with the formulation on automatic, the cost model alone picks the side: the
 *   belief side is no longer taken for memory);  2: always (tests, A/B runs).
 *   chunk_rows: alpha rows per chunk, rounded up to a multiple of 4; 0 = as many as fit (pbvi_gamma_tiling_plan).
 * A request that leaves one chunk runs the untiled path.  Ignored (pbvi_stats_t.gamma_chunks == 1) in dense mode and where
 * Gamma is compact already (fused projection).  An fp64 engine forwards the setting to its fp32 screen.  -1 on bad
 * arguments.  PBVI_GAMMA_TILING=off|auto|always[:rows] in the environment sets the initial mode.
 */
int pbvi_set_gamma_tiling(pbvi_engine_t* e, int mode, int64_t chunk_rows);
/*
 * The planner behind it: pure host arithmetic, callable with no GPU and no engine.  For a model of S states, A actions,
 * O observations, V alpha-vectors against B beliefs, dtype 0 = fp32 / 1 = fp64 scoring, and budget_bytes of device memory
 * for the scoring stage's buffers:
 *   *chunk_rows in: 0 = choose (one chunk when everything fits, else the fewest equal chunks that fit), > 0 = use this
 *               many rows (rounded up to a multiple of 4);  out: rows per chunk (a multiple of 4; >= V with one chunk)
 *   *n_chunks   out: ceil(V / chunk_rows)
 *   *bytes_needed out: an upper bound of the chunk's Gamma rows, its score slabs and GEMM tile lists, plus -- with more
 *               than one chunk -- the full score matrix (one chunk needs none).  Non-decreasing in chunk_rows among tiled
 *               plans.
 * Returns 0, -1 on bad arguments, -2 (with a pbvi_last_error text) when the plan -- a 4-row chunk, if the planner
 * chooses -- exceeds the budget.
 */
int pbvi_gamma_tiling_plan(int32_t S, int32_t A, int32_t O, int64_t V, int64_t B, int dtype, int64_t budget_bytes,
                           int64_t* chunk_rows, int64_t* n_chunks, int64_t* bytes_needed);

/* Tuning knob for f32 engines: relative half-width of the near-tie window that sends an
 * argmax to fp64 refinement (<= 0 restores the default derived from |S|). */
int pbvi_set_tie_window(pbvi_engine_t* e, double rel);

/* Debug aid for tests: when enabled (or PBVI_POISON is set in the environment) every fresh device
 * allocation is filled with 0xFF bytes (NaN floats, -1 indices), so a read of memory the engine never
 * wrote fails the parity tests instead of hiding behind zero-filled pages.  Returns the previous state. */
int pbvi_debug_poison(int enable);
/*
 * The MemoryError contract of src/pomdp.py:2399-2401 ("Memory full ... returning value function and history as is"):
 * a device allocation that fails makes the call return PBVI_ENOMEM (-2), which the Python seam raises as MemoryError and
 * PBVI_Solver.solve turns into the partial result.
 *   pbvi_debug_alloc_limit : cap (MiB, < 0 = none; also PBVI_ALLOC_LIMIT_MB) on the bytes of device buffers ONE engine
 *                            may hold, so that the contract can be tested deterministically; returns the previous cap.
 *   pbvi_engine_after_oom  : after a -2, release every working set, row store and scratch buffer (the model tables stay):
 *                            the engine is as freshly created and usable again.
 */
int64_t pbvi_debug_alloc_limit(int64_t mb);
int pbvi_engine_after_oom(pbvi_engine_t* e);
/* Debug aid for tests of the engines' memory bookkeeping: the bytes of device buffers the library holds right now, over
 * all engines of the process (allocated minus freed).  With one engine alive it equals that engine's pbvi_device_bytes;
 * with none it is 0. */
int64_t pbvi_debug_live_bytes(void);

/* Benchmark / debug: list every K tile of every GEMM tile pair, zero or not -- the "dense backup" configuration of
 * BASELINE.json is measured this way (results are unchanged: skipped tiles only ever add +0).  Also enabled by
 * PBVI_GEMM_DENSE=1 in the environment.  Process-wide; returns the previous state. */
int pbvi_debug_gemm_dense(int enable);
/* Tests only: which K-step schedule the split score GEMM (bf16 MFMAs) runs.  0 (default): each MFMA group
 * reads its LDS fragments right before its MFMAs; 1: fragment reads one MFMA group ahead of their use, behind counted
 * waits.  Same plan, lists, LDS image and accumulation order, so the slabs are bit-identical; the test holds them so.
 * Other values change nothing.  Process-wide; returns the previous schedule.  Not a tuning knob: time a schedule in a
 * build of its own. */
int pbvi_debug_split_schedule(int schedule);
/* Tests and A/B only: whether schedule 0 runs with the block's two wave halves staggered by role (waves 4-7 stage the
 * next tile first and multiply last).  1 (default) or 0; PBVI_NO_SPLIT_STAGGER=1 in the environment starts a
 * process at 0.  Same terms, order and LDS image, so the slabs are bit-identical; the test holds them so.  Schedule 1 has
 * no staggered form and ignores the switch.  Process-wide; returns the previous value. */
int pbvi_debug_split_stagger(int on);
/* Tests only: the raw score slab buffer as the last backup's score GEMM left it (partial slabs in the GEMM plan's layout,
 * padding and parts no block wrote included), copied to host memory.  out == NULL: returns the buffer's size in bytes;
 * else copies that many bytes to out (cap_bytes: the room there) and returns the count.  A stage that runs a GEMM of its
 * own after the scores (belief dominance, the value maxima) re-uses the buffer.  PBVI_EINVAL (negative) when no score GEMM
 * has run or cap_bytes is too small. */
int64_t pbvi_debug_slabs(pbvi_engine_t* e, void* out, int64_t cap_bytes);
/* Tests only: set every byte of that buffer to `byte` (its low 8 bits), so that a test can tell what the next score GEMM
 * wrote from what an earlier one left there.  PBVI_EINVAL when no score GEMM has run. */
int pbvi_debug_slabs_fill(pbvi_engine_t* e, int byte);
/*
 * Tests only: the score probe.  Off by default (one untaken branch in the scoring stage).  While enabled, the scoring
 * stage of every backup (pbvi_backup_run and what is built on it) ends with a copy -- on the pipeline's stream, behind the
 * argmax and in front of the refinement, which rewrites best_v / best_score / E in place -- of what the argmax read and
 * wrote, for the resident B beliefs IN ENGINE ORDER, the G = A * O groups (g = a * O + o) and the V alpha rows:
 *   score      [B][G][V] double  the score the argmax read, through the same slab view (belief-side rows, split-K slabs,
 *                                stream-K continuation tiles, the folded matrix of a Gamma-tiled call)
 *   mag        [B][G]    double  the magnitude score that scales the tie window
 *   E          [B][G]    double  the window, best_v [B][G] int32 and best_score [B][G] double as the argmax wrote them
 *   queue      [qcount]  int32   the near-tie queue as the argmax left it (entries b * G + g, slot order not defined)
 *   dead       [B][G]    uint8   the dead-triple flags the argmax was given (all 0 when it was given none)
 *   perm       [B]       int32   caller's row of engine row b (the resident block's order: fetch before replacing the block)
 *   dims       [8]       int64   B, G, V, qcount, belief-side formulation (0/1), tile pairs of the fp64 MFMA GEMM (0: the
 *                                plain kernel or an fp32 GEMM), its K parts, Gamma chunks (ScoreStage: 0 = belief side)
 *   scalars    [4]       double  split (0/1), chain_steps[0] (-1: none), the tol_rel passed to the argmax (< 0: derived
 *                                on the device from chain_steps), tol_extra
 * An fp64 engine behind its fp32 screen captures the screen's stage (the one whose window decides what is re-decided); a
 * pure fp64 engine its own: E = 0, no queue.  The buffers are working buffers of the engine (pbvi_device_bytes,
 * pbvi_debug_alloc_limit, released by pbvi_engine_after_oom and by disabling the probe).  A backup with
 * B * G * V > 2^24 fails with PBVI_EINVAL while the probe is on.  The Q-value and infotaxis GEMMs are not covered; the value-max
 * GEMMs are pinned from their results (tests/test_value_max.py) and report their route through pbvi_debug_value_max_route.
 * pbvi_debug_score_probe_fetch copies the last capture to host arrays; any pointer may be NULL (call it with dims alone
 * to size the rest).  PBVI_EINVAL when nothing was captured since the probe was enabled.
 */
int pbvi_debug_score_probe(pbvi_engine_t* e, int enable);
int pbvi_debug_score_probe_fetch(pbvi_engine_t* e, int64_t* dims, double* scalars, double* score, double* mag, double* E,
                                 int32_t* best_v, double* best_score, int32_t* queue, uint8_t* dead, int32_t* perm);
/*
 * Tests only: the bookkeeping of the engine's most recent refinement pass (the fp64 re-decision of the near-tie queue
 * of a backup, or of the value maxima of an fp32 engine), so that a test can tell which of its paths ran:
 *   out[0]  candidates reserved on the item list                     (RefineWork::cnt[0]; uncapped: > out[3] = overflow)
 *   out[1]  slots reserved for entries handed to the grid-wide passes (cnt[1]; uncapped: > out[4] = overflow)
 *   out[2]  entries handed to k_refine_split by the level-1 screen    (cnt[2]; uncapped: > out[6] = overflow)
 *   out[3]  item_cap, out[4] slot_cap, out[5] w_slot_cap (slots below it take the GEMM path), out[6] q2_cap,
 *   out[7]  defer_min -- the capacities that pass ran with (all 0 with PBVI_REFINE_INBLOCK: no work list).
 * One 12-byte copy from the counter buffer behind a synchronisation; nothing is recorded per call.  Valid until the
 * next call that refines.  PBVI_EINVAL before the first such pass or once its work list has been released.
 */
int pbvi_debug_refine_counts(pbvi_engine_t* e, int64_t out[8]);
/*
 * Tests only: the route of the engine's most recent value-max GEMM (pbvi_value_max, or the last 32768-row window of
 * pbvi_value_max_store), so that a test can tell which kernels ran:
 *   out[0]  route: 1 = fp32 skinny tile (fp64 accumulation, no window), 2 = fp32 score GEMM with every belief re-scored
 *           in fp64, 3 = fp32 score GEMM as it is (pbvi_set_value_max_exact(0)), 4 = fp64 MFMA GEMM, 5 = fp64 plain kernel
 *   out[1]  column-tile width of that GEMM (16 / 32 / 48 / 64 / 128; 256 for the fp32 score GEMM; 0 for the plain kernel)
 *   out[2]  K parts of the fp64 tile engine (routes 1, 4; 1 for the plain kernel; 0 for the fp32 score GEMM's stream-K walk)
 *   out[3]  belief rows and out[4] alpha rows of that call, out[5] its tile pairs (0 for the plain kernel)
 *   out[6]  value-max GEMMs run since the engine was created (one per window of a store call), out[7] 0
 * Host words only: nothing is read from or kept on the device.  PBVI_EINVAL before the first value-max call.
 */
int pbvi_debug_value_max_route(pbvi_engine_t* e, int64_t out[8]);

/* Bytes of device memory currently held by the handle. */
int64_t pbvi_device_bytes(const pbvi_engine_t* e);

#ifdef __cplusplus
}
#endif
#endif /* PBVI_HIP_H */
