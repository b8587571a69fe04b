// csrc/kernels/launch.h — host-callable launchers of the HIP kernels.  Every
// launcher enqueues on ctx->stream and returns without synchronising.
#pragma once
#include <cstdint>

#include "../common.h"
#include "witness_dev.h"

namespace ipcfp {

// --- blake2b_cid.hip (K1) ---
int launch_chunk_order(ipcfp_ctx* ctx, const uint32_t* len_d, uint32_t n, uint32_t* bins_d, uint32_t* order_d);
int launch_k1_layout(ipcfp_ctx* ctx, const uint32_t* len_d, uint32_t n, uint32_t* bins_d, uint32_t* order_d,
                     uint32_t* sched_len_d, uint64_t* sched_off_d, uint64_t* total_d, uint64_t* scan_scratch_d,
                     uint64_t* off_by_id_d, void* meta_d);
int launch_gather_cids(ipcfp_ctx* ctx, const uint32_t* order_d, const uint8_t* cids_d, uint32_t n, uint8_t* sched_cids_d);
int launch_blake2b256_cid(ipcfp_ctx* ctx, const uint8_t* arena, const void* meta, const uint8_t* sched_cids40, uint32_t n,
                          uint32_t* ok_bits, uint8_t* status, unsigned long long* counters);
int launch_blake2b256_raw(ipcfp_ctx* ctx, const uint8_t* arena, const void* meta, uint32_t n, uint8_t* out32);

// --- repack.hip ---
// new_off[i] = exclusive prefix sum of round_up(len[i], 16); *total_d receives the arena size.
int launch_aligned_offsets(ipcfp_ctx* ctx, const uint32_t* len_d, uint32_t n, uint64_t* new_off_d,
                           uint64_t* total_d, uint64_t* scratch_d /* >= div_up(n,1024)+1 */);
// off[i] = exclusive prefix sum of len[i] (blocks back to back); *total_d = the sum
int launch_tight_offsets(ipcfp_ctx* ctx, const uint32_t* len_d, uint32_t n, uint64_t* off_d, uint64_t* total_d,
                         uint64_t* scratch_d /* >= div_up(n,1024)+1 */);
// cids40[i] = prefix ‖ digests32[i] (zero-padded slot), then the n_esc escape slots as given (ipcfp_witness_create_packed)
int launch_expand_cids(ipcfp_ctx* ctx, const uint8_t* digests32_d, uint32_t n, const uint8_t* prefix, uint32_t prefix_len,
                       const uint32_t* esc_index_d, const uint8_t* esc_cids40_d, uint32_t n_esc, uint8_t* cids40_d);
// dst[new_off[i] .. +len[i]) = src[old_off[i] .. +len[i]); pad bytes up to the next 16 are zeroed.
int launch_repack(ipcfp_ctx* ctx, const uint8_t* src, const uint64_t* old_off, const uint32_t* len,
                  const uint64_t* new_off, uint32_t n, uint8_t* dst);

// --- hash_short.hip (K2 Keccak-256, K3 SHA-256) ---
int launch_keccak256(ipcfp_ctx* ctx, const uint8_t* bytes, const uint64_t* off, const uint32_t* len, uint32_t n,
                     uint8_t* out32);
int launch_sha256(ipcfp_ctx* ctx, const uint8_t* bytes, const uint64_t* off, const uint32_t* len, uint32_t n,
                  uint8_t* out32);

// --- walk.hip (K5 amt_get, K7 hamt_get) ---
int launch_amt_get(ipcfp_ctx* ctx, const WitnessView& w, const CidKey& root, int version, int vkind,
                   const uint64_t* index_d, uint32_t n, uint8_t* status_d, void* loc_d);
int launch_hamt_get(ipcfp_ctx* ctx, const WitnessView& w, const CidKey& root, uint32_t bit_width, int vkind,
                    const uint8_t* keys_d, const uint32_t* key_off_d, const uint32_t* key_len_d, uint32_t n,
                    uint8_t* status_d, void* loc_d, int pending_only = 0);
// --- hamt_levels.hip --- K7 level by level: every visited node decoded once; what it leaves kStPending is the walker's
size_t hamt_levels_scratch_words(uint32_t n, uint32_t n_blocks, uint32_t levels);
int launch_hamt_get_levels(ipcfp_ctx* ctx, const WitnessView& w, const CidKey& root, uint32_t bit_width, int vkind,
                           const uint8_t* keys_d, const uint32_t* key_off_d, const uint32_t* key_len_d, uint32_t n,
                           uint8_t* status_d, void* loc_d, uint32_t levels, uint32_t* scratch_d, void* recs_d, bool coop = true,
                           void* etabs_d = nullptr /* etab_cap × HamtEntryTab (hamt_table.h): the visited nodes' bucket entries */,
                           uint32_t etab_cap = 0);

// --- walk.hip --- K7 over the HAMT node table of a witness (hamt_table.h; the table's kernels: hamt_table_lane.hip below)
uint32_t hamt_kind_bit(int vkind);  // HK_* bit of a value kind, 0: the table does not know that kind
int launch_hamt_get_table(ipcfp_ctx* ctx, const WitnessView& w, const void* table_d, const CidKey& root, uint32_t bit_width,
                          int vkind, const uint8_t* keys_d, const uint32_t* key_off_d, const uint32_t* key_len_d, uint32_t n,
                          uint8_t* status_d, void* loc_d);

// --- verify_storage.hip ---
struct StorageClaimPacked;
int launch_verify_storage(ipcfp_ctx* ctx, ipcfp_witness* w, const StorageClaimPacked* claims_d, uint32_t n,
                          const ipcfp_trust_policy_t& trust, uint8_t* status_d);  // host/verify_storage.cpp
// the pieces of it (verify_storage.hip: runs of claims and their decoded facts; the one-lane kernel)
int launch_storage_run_flags(ipcfp_ctx* ctx, const void* claims_d, uint32_t n, uint32_t* flag_d);
int launch_storage_run_heads(ipcfp_ctx* ctx, const uint32_t* flag_d, const uint32_t* pos_d, uint32_t n, uint32_t* run_of_d, void* runs_d);
int launch_storage_run_facts(ipcfp_ctx* ctx, const WitnessView& w, const void* claims_d, void* runs_d, uint32_t n_runs);
int launch_storage_run_actors_table(ipcfp_ctx* ctx, const WitnessView& w, const void* table_d, const void* claims_d, void* runs_d,
                                    uint32_t n_runs, uint32_t undecided);
int launch_verify_storage_table(ipcfp_ctx* ctx, const WitnessView& w, const void* table_d, const void* claims_d, uint32_t n,
                                const uint32_t* run_of_d, const void* runs_d, uint32_t n_runs, uint32_t* root_children_d,
                                const ipcfp_trust_policy_t& trust, uint32_t undecided, uint8_t* status_d);
int launch_storage_run_actors_lane(ipcfp_ctx* ctx, const WitnessView& w, const void* claims_d, void* runs_d, uint32_t n_runs,
                                   uint32_t undecided);
int launch_verify_storage_lanes(ipcfp_ctx* ctx, const WitnessView& w, const StorageClaimPacked* claims_d, uint32_t n,
                                const ipcfp_trust_policy_t& trust, uint8_t* status_d, int pending_only);

// … the same over the run-compressed column form (storage_runs.h ColumnClaimSrc): the column instantiations of the kernels above
struct ColumnClaimSrc;
struct StorageColumnsDev {  // the form resident in HBM (include/ipcfp.h): run table, columns, counts
    const void* runs;
    uint32_t n_runs;
    const uint8_t *slot, *value, *cflags;
};
int launch_verify_storage_columns(ipcfp_ctx* ctx, ipcfp_witness* w, const StorageColumnsDev& cols, uint32_t n,
                                  const ipcfp_trust_policy_t& trust, uint8_t* status_d, bool wait_upload = false);  // host/verify_storage.cpp
int launch_storage_run_facts(ipcfp_ctx* ctx, const WitnessView& w, const ColumnClaimSrc& cols, void* runs_d, uint32_t n_runs);
int launch_storage_run_actors_table(ipcfp_ctx* ctx, const WitnessView& w, const void* table_d, const ColumnClaimSrc& cols, void* runs_d,
                                    uint32_t n_runs, uint32_t undecided);
int launch_storage_run_actors_lane(ipcfp_ctx* ctx, const WitnessView& w, const ColumnClaimSrc& cols, void* runs_d, uint32_t n_runs,
                                   uint32_t undecided);
int launch_verify_storage_table(ipcfp_ctx* ctx, const WitnessView& w, const void* table_d, const ColumnClaimSrc& cols, uint32_t n,
                                const uint32_t* run_of_d, const void* runs_d, uint32_t n_runs, uint32_t* root_children_d,
                                const ipcfp_trust_policy_t& trust, uint32_t undecided, uint8_t* status_d);
int launch_verify_storage_lanes(ipcfp_ctx* ctx, const WitnessView& w, const ColumnClaimSrc& cols, const uint32_t* run_of_d, uint32_t n,
                                const ipcfp_trust_policy_t& trust, uint8_t* status_d, int pending_only);
// --- storage_columns.hip --- the run table checked (it must tile [0, n): *bad_d |= 1 where it does not) and laid out per claim:
// run_of_d[t] = claim t's run for every run that is sound; runs_d (nullable): StorageRun[n_runs], first_claim set
int launch_storage_column_runs(ipcfp_ctx* ctx, const StorageColumnsDev& cols, uint32_t n, uint32_t* run_of_d, void* runs_d, uint32_t* bad_d);
// columns → StorageClaimPacked[n] (run_of_d as filled above)
int launch_expand_storage_columns(ipcfp_ctx* ctx, const StorageColumnsDev& cols, uint32_t n, const uint32_t* run_of_d, void* claims_out_d);

// --- claims_compact.hip --- compact event claims → EventClaimPacked[n] + blob; scratch_u32: 4 n words, scan_scratch: div_up(n, 1024) + 2
// u64 whose LAST word receives the packed blob's length
int launch_expand_claims(ipcfp_ctx* ctx, const void* compact_d, uint32_t n, const ipcfp_event_claim_group_t* groups_d, uint32_t n_groups,
                         const uint8_t* cblob_d, uint64_t cblob_len, void* claims_out_d, uint8_t* blob_out_d, uint64_t cap_blob,
                         uint32_t* scratch_u32, uint64_t* scan_scratch);

// --- event_claims_gen.hip --- generated matches → EventClaimPacked[n] + blob (ipcfp_event_claims_from_matches_device)
// one lane per match: bounds check, decode_event_log over exactly the item, the claim's blob segment size and its GenRec
// (32 B: where the topics and the data lie, so that the fill decodes nothing); then size_d's prefix sum into off_d / *total_d
// scratch_d: div_up(n, 1024) + 1 u64
int launch_gen_claim_sizes(ipcfp_ctx* ctx, const WitnessView& w, const void* matches_d, uint32_t n, void* recs_d, uint64_t* size_d,
                           uint64_t* off_d, uint64_t* total_d, uint64_t* scratch_d);
// the claim records and the blob's `total` bytes (total < 2^32; blob_out_d holds at least that many)
int launch_gen_claim_fill(ipcfp_ctx* ctx, const WitnessView& w, const void* matches_d, const CidKey* message_d, uint32_t n,
                          const void* recs_d, const uint64_t* off_d, uint64_t total, long long parent_epoch, long long child_epoch,
                          uint32_t tipset, void* claims_out_d, uint8_t* blob_out_d);
// idx_d[i] = matches_d[i].exec_index (generate.hip)
int launch_match_exec_index(ipcfp_ctx* ctx, const void* matches_d, uint32_t n, uint64_t* idx_d);

// --- scan.hip ---
int launch_scan_u32(ipcfp_ctx* ctx, const uint32_t* in_d, uint32_t n, uint32_t* out_d, uint64_t* total_d,
                    uint64_t* scratch_d);
int launch_scan_u64(ipcfp_ctx* ctx, const uint64_t* in_d, uint32_t n, uint64_t* out_d, uint64_t* total_d,
                    uint64_t* scratch_d);

// --- verify_events.hip ---
struct TipsetCtxDev;
struct AmtRootSpec;
struct ReceiptRec;
struct EventRec;
struct EventTableView;
struct LeafRef;
struct EventClaimPacked;
// the header facts of ONE context (tipset_prepare_general.hip; the tipset prologue below is the whole of it)
int launch_ctx_headers(ipcfp_ctx* ctx, const WitnessView& w, TipsetCtxDev* ctx_d);
struct CtxFinish;
// the flags' prefix sum (decoupled look-back), positions (pos_d), inverse, total (total_d) and the context's tail in one
// launch, the flags ready in a.first; ctl_d: exec_scan_ctl_words(a.raw_len) words that are zero when it is queued
int launch_exec_scan_finish(ipcfp_ctx* ctx, TipsetCtxDev* ctx_d, const CtxFinish& a, uint32_t* pos_d, uint64_t* total_d,
                            unsigned long long* ctl_d);
size_t exec_scan_ctl_words(uint32_t n);
int launch_exec_insert_flags(ipcfp_ctx* ctx, const CidKey* keys_d, uint32_t n, unsigned long long* slots_d, uint32_t mask,
                             uint32_t* first_d);
int launch_exec_finish(ipcfp_ctx* ctx, TipsetCtxDev* ctx_d, const uint64_t* total_d, const uint32_t* first_d,
                       const uint32_t* pos_d, uint32_t n, uint32_t* inv_d);
// the tipset prologue (tipset_prepare.hip; launchers and the general companion in tipset_prepare_general.hip)
// jobs_d: device array of {TipsetCtxDev* ctx, AmtRootSpec* roots (nullable), unsigned long long* err}
int launch_tipset_prepare(ipcfp_ctx* ctx, const WitnessView& w, const void* jobs, const void* jobs_d, uint32_t n_jobs,
                          bool need_general, bool defer_rehash = false,  // defer_rehash: see tipset_ctx.h txmeta_block
                          const void* inline_inputs = nullptr);  // host TipsetInputs of the one context: sent as a kernel argument
int launch_exec_roots(ipcfp_ctx* ctx, const WitnessView& w, const TipsetCtxDev* ctx_d, AmtRootSpec* roots_d,
                      unsigned long long* err_d, int verify_txmeta = 1, uint32_t n_parents = 0);
// the prologue's deferred half: the TxMeta re-hashes launch_tipset_prepare(defer_rehash) left behind (tipset_ctx.h
// txmeta_block), on `stream`
int launch_txmeta_rehash(ipcfp_ctx* ctx, hipStream_t stream, const WitnessView& view, const TipsetCtxDev* ctx_d, unsigned long long* err_d);
// the whole prologue of ONE context with a tipset key wider than the inline form (job: host PrepareJob)
int launch_tipset_prepare_wide(ipcfp_ctx* ctx, const WitnessView& w, const void* job, uint32_t n_parents);
int launch_exec_dedup(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* leaves_d, uint32_t n, CidKey* keys_d,
                      unsigned long long* slots_d, uint32_t mask, uint32_t* first_d);
int launch_exec_compact(ipcfp_ctx* ctx, const CidKey* keys_d, uint32_t n, const uint32_t* first_d,
                        const uint32_t* pos_d, CidKey* out_d);
int launch_verify_events(ipcfp_ctx* ctx, const WitnessView& w, const EventClaimPacked* claims_d, uint32_t n,
                         const TipsetCtxDev* ctxs_d, uint32_t n_ctxs, const uint8_t* blob_d, uint64_t blob_len,
                         const ipcfp_trust_policy_t& trust, const ipcfp_event_filter_t* filter, uint8_t* status_d,
                         void* where_d = nullptr, bool tabulated = false);
// --- verify_table.hip --- the claims the event table settles (everything else is left kStPending)
int launch_verify_events_table(ipcfp_ctx* ctx, const WitnessView& w, const EventClaimPacked* claims_d, uint32_t n,
                               const TipsetCtxDev* ctxs_d, uint32_t n_ctxs, const uint8_t* blob_d, uint64_t blob_len,
                               const ipcfp_trust_policy_t& trust, const ipcfp_event_filter_t& filter, int has_filter,
                               uint8_t* status_d, void* where_d);

// --- event_scan.hip (K6 scan, K8 replay bitmap) ---
int launch_scan_pass1(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n,
                      const ipcfp_event_filter_t& filter, int has_actor, uint64_t actor, uint32_t* counts_d,
                      unsigned long long* err_d);
int launch_scan_pass2(ipcfp_ctx* ctx, const WitnessView& w, const CidKey& receipts_root, const LeafRef* receipts_d,
                      uint32_t n, const ipcfp_event_filter_t& filter, int has_actor, uint64_t actor,
                      const uint32_t* counts_d, const uint32_t* offsets_d, void* matches_d, uint64_t matches_cap,
                      uint8_t* has_match_d, uint64_t has_cap, uint64_t has_base = 0,
                      const EventTableView* table = nullptr);
// the event table (event_table.h), step 2: receipt → its block's record (filter nullable: no match counts); the
// receipts the block table does not cover are walked
struct BlockRec;
// k_receipt_walk alone, behind records written elsewhere (k_dense_receipt_leaves)
int launch_receipt_walk(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n,
                        const ipcfp_event_filter_t* filter, int has_actor, uint64_t actor, const ReceiptRec* rrecs_d,
                        uint32_t* counts_d, unsigned long long* err_d, hipStream_t stream);
int launch_receipt_events(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n,
                          const ipcfp_event_filter_t* filter, int has_actor, uint64_t actor, const BlockRec* brecs_d,
                          ReceiptRec* rrecs_d, uint32_t* counts_d, unsigned long long* err_d, hipStream_t stream = nullptr);
// --- block_events.hip --- step 1: every block parsed out of LDS in arena order, on `stream` (meta_d: K1Meta[n])
int launch_block_events(ipcfp_ctx* ctx, hipStream_t stream, const uint8_t* arena, const void* meta_d, uint32_t n,
                        const ipcfp_event_filter_t* filter, int has_actor, uint64_t actor, BlockRec* brecs_d,
                        EventRec* erecs_d, uint32_t cap_events, uint32_t* pool_used_d);
// the scan's tail in one launch (prefix sum by decoupled look-back + map + tabulated matches + results in the mailbox)
int launch_scan_tail_fused(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n, uint64_t dense_first,
                           const ipcfp_event_filter_t& filter, int has_actor, uint64_t actor, const EventTableView& table,
                           const uint32_t* counts_d, uint32_t* offsets_d, void* matches_d, uint64_t matches_cap, uint8_t* has_match_d,
                           uint64_t has_cap, uint64_t has_base, unsigned long long* scratch_d, unsigned long long epoch,
                           const unsigned long long* err_a_d, const unsigned long long* err_b_d, unsigned long long* mailbox_dev,
                           unsigned long long seq);
int launch_count_from_table(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n,
                            const ipcfp_event_filter_t& filter, int has_actor, uint64_t actor, const EventTableView& table,
                            uint32_t* counts_d, unsigned long long* err_d);
// --- event_scan_multi.inc (part of event_scan.hip) --- the two passes for a SET of specs (filter_set.h FsView)
struct FsView;
// PASS 1: counts_d[t] = matches of receipt t over all specs; table (nullable): the event table, else every receipt is walked
int launch_count_multi(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n, const FsView& fs,
                       const EventTableView* table, uint32_t* counts_d, unsigned long long* err_d, unsigned long long* ovf_d);
// the tail of the table route in one launch, as launch_scan_tail_fused (same scratch, same mailbox words; [5] = *ovf_d).
// *ovf_d (zero before PASS 1) is raised when a receipt's count or the total does not fit 32 bits
int launch_scan_tail_multi(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n, uint64_t dense_first,
                           const FsView& fs, const EventTableView& table, const uint32_t* counts_d, uint32_t* offsets_d, void* matches_d,
                           uint32_t* match_spec_d, uint64_t matches_cap, uint8_t* has_match_d, uint64_t has_cap, uint64_t has_base,
                           unsigned long long* spec_counts_d, unsigned long long* scratch_d, unsigned long long epoch,
                           const unsigned long long* err_d, unsigned long long* ovf_d, unsigned long long* mailbox_dev,
                           unsigned long long seq);
// PASS 2: the any-spec map, matches_d / match_spec_d (nullable together) at offsets_d, spec_counts_d[n_specs] += per-spec totals.
// tail_done: launch_scan_tail_multi has served the tabulated receipts — only the receipts the table leaves to the walk
int launch_fill_multi(ipcfp_ctx* ctx, const WitnessView& w, const CidKey& receipts_root, const LeafRef* receipts_d, uint32_t n,
                      const FsView& fs, const uint32_t* counts_d, const uint32_t* offsets_d, void* matches_d, uint32_t* match_spec_d,
                      uint64_t matches_cap, uint8_t* has_match_d, uint64_t has_cap, uint64_t has_base,
                      unsigned long long* spec_counts_d, const EventTableView* table, bool tail_done);

// --- event_scan_tipsets.inc (part of event_scan.hip) --- the two passes over the concatenated leaves of T receipts trees
struct AmtRootSpec;
// first_d[s] (s = 0 … n_tipsets): position of the first leaf with seq >= s; n == 0 is served (every entry 0)
int launch_tipset_bounds(ipcfp_ctx* ctx, const LeafRef* leaves_d, uint32_t n, uint32_t n_tipsets, uint32_t* first_d);
// PASS 1 as launch_count_multi with one error word per tipset (err_d[n_tipsets], kNoEnumError each), then the counts of
// every leaf of a tipset whose word is set are zeroed
int launch_count_tipsets(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n, const FsView& fs,
                         const EventTableView* table, uint32_t* counts_d, unsigned long long* err_d, uint32_t n_tipsets,
                         unsigned long long* ovf_d);
// behind launch_scan_u32: per tipset the size of its map (last index + 1) and the record offset at its first leaf
int launch_tipset_shapes(ipcfp_ctx* ctx, const LeafRef* leaves_d, uint32_t n, const uint32_t* first_d, const uint32_t* offsets_d,
                         const uint64_t* total_d, uint32_t n_tipsets, uint64_t* n_idx_d, uint64_t* match_start_d);
// PASS 2 as launch_fill_multi: the map byte of a leaf at receipt_off_d[seq] + index (n_tipsets + 1 offsets; has_cap bounds the
// concatenated map), the recorder's receipts root from roots_d[seq]
int launch_fill_tipsets(ipcfp_ctx* ctx, const WitnessView& w, const AmtRootSpec* roots_d, const unsigned long long* err_d,
                        const uint64_t* receipt_off_d, uint32_t n_tipsets, const LeafRef* receipts_d, uint32_t n, const FsView& fs,
                        const uint32_t* counts_d, const uint32_t* offsets_d, void* matches_d, uint32_t* match_spec_d,
                        uint64_t matches_cap, uint8_t* has_match_d, uint64_t has_cap, unsigned long long* spec_counts_d,
                        const EventTableView* table);

// --- base64.hip ---
int launch_base64_decode(ipcfp_ctx* ctx, const uint8_t* text_d, const void* spans_d, uint32_t n_blocks, uint32_t n_units,
                         const uint64_t* dst_off_d, uint8_t* arena_d, unsigned long long* first_bad_d);

int launch_parse_cid_arrays(ipcfp_ctx* ctx, const uint8_t* text_d, const void* spans_d, uint32_t n, uint8_t* cids_d,
                            unsigned long long* first_bad_d);

// --- base64_encode.hip --- the `blocks` part of a bundle's JSON text out of the witness (host/bundle_write.cpp)
// per list position (ids_d nullable: the identity list): EncPos records (16 B each), text sizes and their exclusive prefix,
// the 16-character unit prefix; totals_d = [text bytes, units]; *first_bad_d = min over (position << 2 | code),
// code 1: id out of range, 2: folded CID slot, 3: slot is not one CID + zero padding; scratch_d: 2·(div_up(n,1024)+1) u64
int launch_bundle_block_sizes(ipcfp_ctx* ctx, const uint32_t* ids_d, uint32_t n, uint32_t n_witness, const uint64_t* off_d,
                              const uint32_t* len_d, const uint8_t* cids_d, void* pos_d, uint64_t* size_d, uint32_t* units_d,
                              uint64_t* text_off_d, uint32_t* unit0_d, uint64_t* totals_d, uint64_t* scratch_d,
                              unsigned long long* first_bad_d);
// the frames of every position and the base64 bodies into text_d (totals_d[0] bytes)
int launch_bundle_write_text(ipcfp_ctx* ctx, const uint32_t* ids_d, uint32_t n, const uint8_t* arena_d, const uint8_t* cids_d,
                             const void* pos_d, const uint64_t* text_off_d, const uint32_t* unit0_d, uint32_t n_units,
                             uint8_t* text_d);

// --- claim_text.hip --- the claims head of a bundle's JSON text out of packed claims in HBM (host/bundle_write_packed.cpp)
constexpr uint32_t kClaimTextRunFragStride = 448;  // bytes of run_frag_d per run
constexpr uint32_t kClaimTextRunInfo = 8;          // bytes of run_info_d per run
constexpr uint32_t kClaimTextTipsetRec = 16;       // tipsets_d: {u64 offset into tipset_frag_d, u32 length, u32 refusal code (0, 7: invalid, 8: folded)}
struct ClaimTextIn {
    StorageColumnsDev cols;    // the storage claims
    uint32_t n_storage;
    const uint32_t* run_of_d;  // launch_storage_column_runs over n_storage words preset to 0xff
    void* run_info_d;          // scratch: n_runs × kClaimTextRunInfo
    uint8_t* run_frag_d;       // scratch: n_runs × kClaimTextRunFragStride
    const void* claims_d;      // EventClaimPacked[n_events]
    uint32_t n_events;
    const uint8_t* blob_d;
    uint64_t blob_len;
    const void* tipsets_d;     // n_tipsets records of kClaimTextTipsetRec
    const uint8_t* tipset_frag_d;
    uint32_t n_tipsets;
};
// per-run fragments, then one lane per item (n_storage + n_events + 3: the three literals of the head are items): checks and
// text sizes into size_d, their exclusive prefix into off_d, *total_d = the head's length.  *first_bad_d (0xff… before) = min
// over (kind << 36 | claim index << 4 | code), kind 0: storage, 1: events; scratch_d: div_up(items, 1024) + 1 u64
int launch_claim_text_sizes(ipcfp_ctx* ctx, const ClaimTextIn& in, uint64_t* size_d, uint64_t* off_d, uint64_t* total_d,
                            uint64_t* scratch_d, unsigned long long* first_bad_d);
// the head_len bytes of the head at text_d (16-byte aligned); only behind a sizing pass that refused nothing
int launch_claim_text_write(ipcfp_ctx* ctx, const ClaimTextIn& in, const uint64_t* off_d, uint64_t head_len, uint8_t* text_d);

// --- generate.hip ---
int launch_generate_storage(ipcfp_ctx* ctx, const WitnessView& w, const CidKey& child, const void* specs_d, uint32_t n,
                            void* out_d);
int launch_mark_cids(ipcfp_ctx* ctx, const WitnessView& w, const CidKey* keys_d, uint32_t n, uint32_t* missing_d);
int launch_gather_keys(ipcfp_ctx* ctx, const CidKey* table_d, uint64_t table_len, const uint64_t* index_d, uint32_t n,
                       CidKey* out_d, uint32_t* oor_d);
int launch_gather_block_cids(ipcfp_ctx* ctx, const uint8_t* cids_d, const uint32_t* ids_d, uint32_t n, CidKey* out_d);

// --- storage_claims_gen.hip --- generate_storage_proof as column claims, over runs of specs with equal actor_id
// (ipcfp_generate_storage_claims*, host/generate.cpp).  `w` of a kernel that fetches blocks: the RECORDING view.
// flag_d[t] = 1 where a run starts (then launch_scan_u32 and launch_storage_run_heads: run_of_d, StorageRun::first_claim)
int launch_sgen_run_flags(ipcfp_ctx* ctx, const uint64_t* actor_id_d, uint32_t n, uint32_t* flag_d);
// child header → parent_state_root → StateRoot.actors; actor_status = `undecided` where the actor get is due
int launch_sgen_run_chain(ipcfp_ctx* ctx, const WitnessView& w, const CidKey& child, void* runs_d, uint32_t n_runs, uint32_t undecided);
// the actor get: over the node table (table_d, nullable), then the walker for every run still undecided
int launch_sgen_run_actors(ipcfp_ctx* ctx, const WitnessView& w, const void* table_d, const uint64_t* actor_id_d, void* runs_d,
                           uint32_t n_runs, uint32_t undecided);
// EVM state behind the derived actor-state CID, layout sniff of the derived contract_state
int launch_sgen_run_state(ipcfp_ctx* ctx, const WitnessView& w, void* runs_d, uint32_t n_runs);
// value_d[32 t], cflags_d[t], status_d[t] of every spec: with a table (table_d, nullable) the first step of every run's get
// resolved once (root_children_d: n_runs × 33 words of scratch) and the table kernel, then the one-lane kernel for what that
// left pending — or for every spec
int launch_sgen_specs(ipcfp_ctx* ctx, const WitnessView& w, const void* table_d, const uint8_t* slot_d, uint32_t n, const uint32_t* run_of_d,
                      const void* runs_d, uint32_t n_runs, uint32_t* root_children_d, uint8_t* value_d, uint8_t* cflags_d,
                      uint8_t* status_d);
// out_d: n_runs records of IPCFP_SRUN_BYTES
int launch_sgen_run_records(ipcfp_ctx* ctx, const void* runs_d, uint32_t n_runs, uint32_t n, const CidKey& child, long long child_epoch,
                            const uint64_t* actor_id_d, void* out_d);
// --- storage_claims_gen_tipsets.inc (part of storage_claims_gen.hip) --- the same for ONE spec list at each of n_tipsets
// children: the kernels above instantiated over SgenChain instead of SgenOne (storage_claims_gen_body.h), behind
// k_sgent_heads and k_sgent_run_init, and the cut.  `w`: the view whose `touched` is row 0 of the recorder, n_tipsets rows of `words` words; runs0_d / run_of0_d:
// launch_storage_run_heads over the n_specs-entry list (n_runs0 runs); runs_d: StorageRun[n_tipsets * n_runs0], run (t, r) at
// t * n_runs0 + r; claim (t, s) at t * n_specs + s
// heads_d (96 bytes per tipset): child header → parent_state_root → StateRoot.actors once per tipset, then every run from it
int launch_sgent_runs(ipcfp_ctx* ctx, const WitnessView& w, uint32_t words, const CidKey* children_d, uint32_t n_tipsets,
                      const void* runs0_d, uint32_t n_runs0, uint32_t n_specs, void* heads_d, void* runs_d, uint32_t undecided);
// the actor get (table_d nullable, then the walker), the EVM state and the layout sniff
int launch_sgent_run_actors(ipcfp_ctx* ctx, const WitnessView& w, uint32_t words, const void* table_d, const uint64_t* actor_id_d,
                            const void* runs0_d, uint32_t n_runs0, uint32_t n_specs, uint32_t n_tipsets, void* runs_d, uint32_t undecided);
// as launch_sgen_specs; slot_d: the n_specs-entry column, slot_out_d: the handle's, written replicated
int launch_sgent_specs(ipcfp_ctx* ctx, const WitnessView& w, uint32_t words, const void* table_d, const uint8_t* slot_d,
                       const uint32_t* run_of0_d, uint32_t n_specs, uint32_t n_runs0, uint32_t n_tipsets, const void* runs_d,
                       uint32_t* root_children_d, uint8_t* slot_out_d, uint8_t* value_d, uint8_t* cflags_d, uint8_t* status_d);
int launch_sgent_run_records(ipcfp_ctx* ctx, const void* runs_d, const void* runs0_d, uint32_t n_runs0, uint32_t n_specs, uint32_t n_tipsets,
                             const CidKey* children_d, const long long* epochs_d, const uint64_t* actor_id_d, void* out_d);
// out_d[words] = the OR of the rows
int launch_sgent_union(ipcfp_ctx* ctx, const uint32_t* rows_d, uint32_t n_tipsets, uint32_t words, uint32_t* out_d);
// the per-tipset lists in the order of union_ids_d (n_union > 0 ids): per (tipset, 32 positions) a mask and its popcount,
// their prefix sum (mask_d, count_d, offset_d: n_tipsets * div_up(n_union, 32) words; scratch_d as launch_scan_u32) …
int launch_sgent_cut_count(ipcfp_ctx* ctx, const uint32_t* rows_d, uint32_t n_tipsets, uint32_t words, uint32_t n_blocks,
                           const uint32_t* union_ids_d, uint32_t n_union, uint32_t* mask_d, uint32_t* count_d, uint32_t* offset_d,
                           uint64_t* total_d, uint64_t* scratch_d);
// … and the lists themselves: ids_out_d[cap], tipset_off_d[n_tipsets + 1]
int launch_sgent_cut_fill(ipcfp_ctx* ctx, const uint32_t* mask_d, const uint32_t* offset_d, const uint64_t* total_d, uint32_t n_tipsets,
                          const uint32_t* union_ids_d, uint32_t n_union, uint64_t cap, uint32_t* ids_out_d, uint64_t* tipset_off_d);

// --- event_gen_tipsets.inc (part of tipset_prepare_general.hip) --- generate_event_proof for a CHAIN of tipset pairs
// (ipcfp_generate_event_claims_tipsets, host/generate.cpp).  tips_d: GentTipset[n_tipsets], facts_d: GentFacts[n_tipsets]
// (host/generate.cpp mirrors both records); `w` of a kernel that fetches blocks: the RECORDING view.
// the chain prologue: ctxs_d TipsetCtxDev[n_tipsets] (inputs set), n_slots = Σ (2 + n_parents) workgroups; roots_d: Σ 2·n_parents
// specs with seq = their number in the chain; err_d[n_tipsets] (kNoEnumError each): stage 1's error word per tipset
int launch_gent_prologue(ipcfp_ctx* ctx, const WitnessView& w, void* ctxs_d, const void* tips_d, uint32_t n_tipsets, uint32_t n_slots,
                         AmtRootSpec* roots_d, unsigned long long* err_d, void* facts_d);
int launch_gent_skip_roots(ipcfp_ctx* ctx, AmtRootSpec* roots_d, uint32_t lo, uint32_t hi);
// leaves → keys_d[n], tip_d[n] (seq_tipset_d: root number → tipset), then the one-probe first-occurrence flags of (tipset, CID)
// (slots_d: mask + 1 words of 0xff, first_d: n zeroed words)
int launch_gent_exec_order(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* leaves_d, uint32_t n, const uint32_t* seq_tipset_d,
                           uint32_t n_roots, CidKey* keys_d, uint32_t* tip_d, unsigned long long* slots_d, uint32_t mask,
                           uint32_t* first_d);
// behind launch_scan_u32 over the flags: exec_off_d[n_tipsets + 1]; first_by_root_d: launch_tipset_bounds over the root numbers
int launch_gent_exec_ranges(ipcfp_ctx* ctx, const void* tips_d, uint32_t n_tipsets, const uint32_t* first_by_root_d, const uint32_t* pos_d,
                            const uint64_t* total_d, uint32_t n, uint32_t* exec_off_d);
// msg_d[k] = list_d[exec_off[t] + exec_index] for match k of tipset t (match_off_d: n_tipsets + 1); oor_d[t] |= 1 when outside
int launch_gent_gather(ipcfp_ctx* ctx, const void* matches_d, uint32_t n, const uint64_t* match_off_d, uint32_t n_tipsets,
                       const uint32_t* exec_off_d, const CidKey* list_d, CidKey* msg_d, uint32_t* oor_d);
// launch_mark_cids with missing_d[key_tip_d[i]] |= 1
int launch_gent_mark_base(ipcfp_ctx* ctx, const WitnessView& w, const CidKey* keys_d, const uint32_t* key_tip_d, uint32_t n,
                          uint32_t* missing_d);
// claim k of tipset t (claim_off_d: n_tipsets + 1): tipset = t and the tipset's two epochs
int launch_gent_patch_claims(ipcfp_ctx* ctx, void* claims_d, uint32_t n, const uint64_t* claim_off_d, uint32_t n_tipsets,
                             const long long* parent_epoch_d, const long long* child_epoch_d);

// --- shard.hip ---
int launch_plan_receipts(ipcfp_ctx* ctx, const WitnessView& rec, const CidKey& receipts_root, uint64_t lo, uint32_t n);
int launch_plan_receipts_all(ipcfp_ctx* ctx, const WitnessView& rec, const CidKey& receipts_root, uint32_t n,
                             const uint64_t* bounds_d, uint32_t n_shards, uint32_t words);
int launch_find_blocks(ipcfp_ctx* ctx, const WitnessView& w, const CidKey* keys_d, uint32_t n, uint32_t* ids_d);
int launch_gather_values(ipcfp_ctx* ctx, const WitnessView& w, const void* locs_d /* ipcfp_value_loc_t[n] */, uint32_t n,
                         uint8_t* out_d, uint64_t stride, unsigned long long* first_bad_d);
int launch_absolute_offsets(ipcfp_ctx* ctx, const uint64_t* off_d, uint32_t n, uint64_t base, uint64_t* out_d);
int launch_amt_root_info(ipcfp_ctx* ctx, const WitnessView& w, const CidKey& root, int version, int vkind, uint64_t* out_d);
int launch_subset_tables(ipcfp_ctx* ctx, const uint32_t* ids_d, uint32_t n, uint32_t n_src, const uint64_t* src_off,
                         const uint32_t* src_len, const uint8_t* src_cids, uint64_t* off_d, uint32_t* len_d,
                         uint8_t* cids_d, uint32_t* bad_d);

int launch_claims_window(ipcfp_ctx* ctx, const void* claims_d, uint32_t n, unsigned long long* win_d);         // claims_compact.hip
// --- the per-call HAMT node table (hamt_table_lane.hip, hamt_levels.hip): one lane per block shorter than `below_len`
// (the storage call: kHamtOutlineMinLen, the 32-lane outline and _rest take the longer ones; ipcfp_hamt_get*'s table: ~0) ---
int launch_hamt_list_long(ipcfp_ctx* ctx, const void* meta_d, uint32_t n, uint32_t* work_d, uint32_t* count_d);
int launch_hamt_outline_list(ipcfp_ctx* ctx, hipStream_t stream, const WitnessView& w, void* recs_d, uint32_t* work_d, uint32_t* count_d,
                             uint32_t bound);
int launch_hamt_node_table_lane(ipcfp_ctx* ctx, const uint8_t* arena, const void* meta_d, uint32_t n, uint32_t below_len, uint32_t kinds,
                                void* recs_d);
int launch_hamt_node_table_rest(ipcfp_ctx* ctx, hipStream_t stream, const WitnessView& w, const uint32_t* work_d, const uint32_t* count_d,
                                uint32_t bound, uint32_t kinds, void* recs_d);
int launch_rebase_claims(ipcfp_ctx* ctx, void* claims_d, uint32_t n, uint64_t base, uint64_t blob_len, uint64_t full_len,
                         uint32_t* miss_d, uint32_t* order_d = nullptr, uint64_t key_lo = 0, uint64_t key_hi = ~0ull);  // claims_compact.hip
// --- shard_pull.hip (shard_pull.h) --- a rank pulls its shard out of a bundle in host memory, level by level
struct PullSeeds;
struct PullFrontier;
struct PullTables;
struct PullCtl;
int launch_pull_seed(ipcfp_ctx* ctx, const WitnessView& w, const PullSeeds& seeds, const PullFrontier& first, PullCtl* ctl_d);
int launch_pull_round(ipcfp_ctx* ctx, const WitnessView& w, const uint8_t* host_bytes_dev, const PullTables& t, const PullFrontier& cur,
                      uint32_t n_items, const PullFrontier& next, PullCtl* ctl_d, uint32_t n_shards, uint32_t shard,
                      unsigned long long* mailbox_dev, unsigned long long seq);
// --- cid_index.hip --- the CID → block table over any (cids, n): slots_d holds mask + 1 words, cleared to 0xff by the caller
int launch_index_insert(ipcfp_ctx* ctx, const uint8_t* cids_d, uint32_t n, uint32_t* slots_d, uint32_t mask);

// device view of a witness (host helper, witness.cpp)
WitnessView witness_view(const ipcfp_witness* w, uint32_t* touched_bits = nullptr);

}  // namespace ipcfp
