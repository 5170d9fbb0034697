// Launch / host entry points of lp_kernels.hip (bound to Python in csrc/bind.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "lp_core.h"

namespace lp {

// worker threads of the host twins (CPU backend)
void set_host_threads(int n);
// lanes per gram hit of the bulk literal verify (k_pf_verify; A/B knob, default 4)
void set_pf_verify_lanes(int n);
// bulk scan walk: hot blocks re-walked by a second kernel (k_scan_rare) instead of inline (A/B knob)
bool scan_defer_rare();
void set_scan_defer_rare(bool on);
// request path: BPG and DFA candidates verified in ONE launch (k_bpg_coop mode 2, default) or in
// two (k_cand_verify, then the BPG walk) -- the diagnostic split shows each half's time
void set_cand_verify_split(bool on);
// event top-k by threshold selection (summarize.hip k_sel_*, default) or the chunk-sort levels
bool summ_select();
void set_summ_select(bool on);
// diagnostic: phase clocks of k_hits_small / k_events_small into a device int64[16] (0: off)
void set_small_profile(uint64_t dev_ptr);
// line-index pass 1 folded into the bulk prefilter (line_index.hip k_nl_count's outputs): per 16 KiB
// tile the '\n' count and the "\r\n" flag (both zeroed by the caller), per 64 bytes a '\n' bitmask
struct NlOut {
  uint64_t* nlm = nullptr;   // [ntiles * 256]
  int32_t* cnt = nullptr;    // [ntiles]
  int32_t* crf = nullptr;    // [ntiles]
  int64_t ntiles = 0;
};
void prefilter_dev(const uint8_t* text, int64_t nbytes, const PfTables& T, const int64_t* line_start, int64_t nlines,
                   int64_t* cand, int64_t cap, unsigned long long* count, int grid, uint64_t stream,
                   const NlOut* nl = nullptr);
void pf_verify_dev(const int64_t* ghits, int64_t n, const uint8_t* text, int64_t nbytes, const PfTables& T,
                   const int64_t* line_start, int64_t nlines, const int32_t* blk_line, int64_t* cand, int64_t cap,
                   unsigned long long* count, uint64_t stream, const unsigned long long* dn = nullptr,
                   int max_grid = 8192);
// bit-parallel Glushkov programs (bpg.hip): candidate verify (small path, in place), first-of-run
// verify of sorted keys (bulk path, flags), all-lines scan of literal-free programs
void bpg_cand_dev(int64_t* cand, int64_t cap, const unsigned long long* dcount, const uint8_t* text, const int64_t* ls,
                  const int32_t* ll, const DfaPool& P, uint64_t stream);
// request path: DFA candidates (grid's upper half) and BPG candidates (lower half, cooperative walk)
// verified in place by ONE launch; false (nothing launched) when the library has no BPG programs
bool cand_verify_all_dev(int64_t* cand, int64_t cap, const unsigned long long* dcount, const uint8_t* text,
                         const int64_t* ls, const int32_t* ll, const DfaPool& P, uint64_t stream);
// wcnt / wlist (optional): a counter zeroed in stream order before the call and n uint32 of scratch --
// keys of programs wider than 8 words are listed there and walked one lane group per key
// std_key (optional): the DFA dedupe-verify of every key (k_dedupe_verify's flag / std_key) runs in
// the same launch; returns false when nothing was launched (no BPG program) -- the caller then runs
// the DFA dedupe-verify itself
bool bpg_dedupe_dev(const uint64_t* keys, int64_t n, int lbits, const uint8_t* text, const int64_t* ls,
                    const int32_t* ll, const DfaPool& P, uint8_t* flag, uint64_t stream, uint32_t* wcnt = nullptr,
                    uint32_t* wlist = nullptr, int64_t* std_key = nullptr);
void bpg_scan_dev(const uint8_t* text, const int64_t* ls, const int32_t* ll, int64_t L, const int32_t* regs,
                  int nregs, const DfaPool& P, int64_t* out, int64_t cap, unsigned long long* count,
                  uint64_t stream);
// backtracker regexes fed by their relaxed automata (side_path.hip): export of the candidates to
// pinned host memory (keys / starts / lens / host_cnt / host_seq are device-visible pointers of
// pinned host memory; cnt / done_blocks device words, zero between uses). keys == null: drop mode.
struct HostSideOut {
  int64_t* keys = nullptr;
  int64_t* starts = nullptr;
  int64_t* lens = nullptr;
  int64_t cap = 0;
  unsigned long long* cnt = nullptr;
  unsigned int* done_blocks = nullptr;
  int64_t* host_cnt = nullptr;
  int64_t* host_seq = nullptr;
  int64_t seq = 0;
};
// ... and the host's verified keys (pinned, device-visible), published with host_seq == seq
struct HostSideIn {
  const int64_t* keys = nullptr;
  const int64_t* host_cnt = nullptr;
  const int64_t* host_seq = nullptr;
  int64_t cap = 0;
  int64_t seq = 0;
  long long timeout_ticks = 200000000;   // wall_clock64 ticks (100 MHz): 2 s
  int64_t* err = nullptr;                // set to 1 when the host did not answer in time
};
void take_host_dev(int64_t* cand, const unsigned long long* n1d, int64_t cap1, int64_t* ver,
                   const unsigned long long* n2d, int64_t cap2, const uint8_t* text, const int64_t* ls,
                   const int32_t* ll, const DfaPool& P, const HostSideOut& O, uint64_t stream);
void wait_host_dev(int64_t* ver, int64_t cap2, unsigned long long* n2d, const HostSideIn& I, uint64_t stream);

// host-verified keys appended to a verified-hit buffer at its device counter (k_append_keys)
void append_keys_dev(int64_t* dst, int64_t cap, unsigned long long* count, const int64_t* src, int64_t n,
                     uint64_t stream);
void scan_dev(const uint8_t* text, const int64_t* line_start, const int32_t* line_len, int64_t nlines,
              const int32_t* regs, int nregs, const DfaPool& P, int64_t* out, int64_t cap, unsigned long long* count,
              uint64_t stream);
void score_dev(const int32_t* ev_line, const int32_t* ev_pat, const int32_t* ev_seg, const FreqIn& F, int64_t n,
               const ScoreTables& T, const ScoreParams& S, double* out, double* factors, uint64_t stream,
               const int64_t* dn = nullptr);   // dn: device event count (n = capacity)

void seq_chain_dev(const int32_t* slot_seq, const int32_t* seq_ev_off, const int32_t* seq_ev_reg,
                   const int64_t* hit_off, const int32_t* hit_line, int32_t own_lo, int32_t own_hi, int nslots,
                   int32_t* out, uint64_t stream);
void seq_chain_host(const int32_t* slot_seq, const int32_t* seq_ev_off, const int32_t* seq_ev_reg,
                    const int64_t* hit_off, const int32_t* hit_line, int32_t own_lo, int32_t own_hi, int nslots,
                    int32_t* out);
int64_t nl_positions_host(const uint8_t* text, int64_t nbytes, int64_t* nl_pos);
// AVX-512 bloom tier of the host twin (prefilter_cpu.cpp): 4-gram-only bloom, no Teddy tier;
// handles positions from the 4-aligned point at or after `a` in 64-byte steps, returns where it stopped
bool prefilter_bloom_simd_ok();
int64_t prefilter_bloom_simd(const uint8_t* text, int64_t nbytes, const PfTables& T, const int64_t* line_start,
                             int64_t nlines, int64_t a, int64_t b, std::vector<int64_t>& out);
int64_t prefilter_teddy_simd(const uint8_t* text, int64_t nbytes, const PfTables& T, const int64_t* line_start,
                             int64_t nlines, int64_t a, int64_t b, std::vector<int64_t>& out);
int64_t prefilter_host(const uint8_t* text, int64_t nbytes, const PfTables& T, const int64_t* line_start,
                       int64_t nlines, int64_t* cand, int64_t cap);
int64_t scan_host(const uint8_t* text, const int64_t* line_start, const int32_t* line_len, int64_t nlines,
                  const int32_t* regs, int nregs, const DfaPool& P, int64_t* out, int64_t cap);
void score_host(const int32_t* ev_line, const int32_t* ev_pat, const int32_t* ev_seg, const FreqIn& F, int64_t n,
                const ScoreTables& T, const ScoreParams& S, double* out, double* factors);

}  // namespace lp

namespace lp {
void nfa_mfma_dev(const uint64_t* groups, const int32_t* group_list, int ngroups, int ncls, const int32_t* lines,
                  int64_t nsel, const uint8_t* text, const int64_t* line_start, const int32_t* line_len,
                  uint8_t* feat, int64_t* hits, int64_t cap, unsigned long long* count, uint64_t stream);
int64_t nfa_host(const uint64_t* groups, const int32_t* group_list, int ngroups, const int32_t* lines, int64_t nsel,
                 const uint8_t* text, const int64_t* line_start, const int32_t* line_len, uint8_t* feat,
                 int64_t* hits, int64_t cap);
}  // namespace lp

// ---- literal-free scan (scan_multi.hip): up to 4 multi-regex DFA groups per pass, tables in LDS
namespace lp {
struct ScanPass {
  const uint32_t* blob;   // device (or host) copy of the whole blob; layout in scan_multi.hip
  int lds_words;          // leading words staged in LDS: u16 rows + bm4 (multiple of 4)
  int ngroups;            // 1..4
  int row_base[4];        // u16 index of group g's first row
  int stride[4];          // row stride (u16 entries, odd)
  int thr[4];             // first row index of a state from which a regex can accept
  int init_row[4];        // row index of the start state
  uint32_t init_state[4]; // start state id (exact tables)
  int ncol[4];            // columns: hold, '\n', byte classes
  int gt_off[4];          // word offset of group g's exact [state][ncol] next-state table
  int gm_off[4];          // word offset of group g's [state][ncol] accept masks (same indexing)
  int fin_off[4];         // word offset of group g's [state][EOL, FT] accept masks
  int bm_off;             // word offset of bm4
  int rid_off;            // word offset of the regex ids (64 per group)
  int am_off;             // word offset (even) of the u64 accept masks laid out like the LDS rows
};
void scan_multi_dev(const uint8_t* text, int64_t nbytes, const int64_t* line_start, const int32_t* line_len, int64_t nlines,
                    const ScanPass& S, int64_t* out, int64_t cap, unsigned long long* count, int grid,
                    uint64_t stream);
int64_t scan_multi_host(const uint8_t* text, const int64_t* line_start, const int32_t* line_len, int64_t nlines,
                        const ScanPass& S, int64_t* out, int64_t cap);
}  // namespace lp

// ---- device-resident frequency state (freq_state.hip)
namespace lp {
struct FreqRing {
  double* t;          // [cap] batch timestamps (seconds)
  int32_t* key;       // [cap] frequency key
  int32_t* cnt;       // [cap] matches of the key in that batch
  int64_t cap;
  int64_t* ht;        // [2] head, tail positions (monotonic)
  int64_t* tot;       // [K] in-window matches per key
  uint8_t* seen;      // [K]
};
void freq_evict(const FreqRing& R, double horizon, uint64_t stream, bool dev);
// gate (device, optional): record only when cnt[0..2] <= cap[0..2] and cnt[4] <= cap[3] -- the
// request runner's matcher / event capacities held, so the counts are this batch's real ones
struct RecordGate {
  const int64_t* cnt = nullptr;
  int64_t cap[4] = {0, 0, 0, 0};
  const int64_t* veto = nullptr;   // (device) record only when *veto == 0: a DP step's overflow veto
};
void freq_record(const int64_t* counts, int K, double now, const FreqRing& R, uint64_t stream, bool dev,
                 const RecordGate& gate = RecordGate());
}  // namespace lp

// ---- line index (line_index.hip)
namespace lp {
struct LineIndexWs {
  int64_t* buf;                // [4 * ntiles_cap] tile offsets, first line ends (line, end), counts;
  int64_t ntiles_cap;          // then tmp_bytes of scan scratch
  size_t tmp_bytes;
};
int64_t line_index_tiles(int64_t nbytes);
// starts/lens [cap]; info[0] = '\n' count, info[1] = last '\n' (or -1), info[2] = lines after
// Java's trailing-empty trimming (trim only). Lines = info[0] + 1 before trimming.
// blk (optional) [nblk]: line holding byte b << 12 (the coarse index of lp_core.h locate_line)
void line_index_dev(const uint8_t* text, int64_t nbytes, const LineIndexWs& W, int64_t* starts, int32_t* lens,
                    int64_t cap, int64_t* info, bool trim, int32_t* blk, int64_t nblk, uint64_t stream,
                    bool counted = false);
// the workspace views pass 1 writes (counted = true: a fused prefilter already wrote them); zeroes
// the counts and flags on `stream`
NlOut line_index_pass1_views(const LineIndexWs& W, int64_t nbytes, uint64_t stream);
}  // namespace lp

// ---- DP step bookkeeping (dp_glue.hip)
namespace lp {
struct DpCarryArgs {
  const int64_t* g;          // [world][1 + nk + ns] gathered payloads
  int world, rank, nk, ns;
  int64_t halo_left;
  const int64_t* tot;        // [nk] persistent window totals (may be null)
  const int64_t* slot_e0;    // [ns] first slot of each sequence-event slot's sequence
  const int64_t* slot_k;     // [ns] event index of the slot
  // outputs
  int64_t* own_start; int64_t* g0; int64_t* n;   // [1] each
  int64_t* carry;            // [nk]
  uint8_t* seq_carry;        // [ns]
  int64_t* red_tail;         // [nk] this rank's counts into the all-reduce buffer (may be null)
  int64_t* veto = nullptr;   // [1] OR of every rank's overflow flag (may be null)
  int64_t* zero = nullptr;   // [nzero] zeroed (this rank's histogram slots of the all-gather buffer)
  int64_t nzero = 0;
  // a stream of DP steps (parallel/stream.py ShardedStreamAnalyzer): the carries of the earlier
  // steps -- sequence-chain state before this step, global index of its first line, an open N
  // (chronological factor rescored at the end) -- and the state after the step (every rank composed)
  const uint8_t* seq_base = nullptr;   // [ns] or null (= nothing matched before the step)
  int64_t line_base = 0;
  int64_t n_fixed = 0;                 // > 0: N written as this instead of the step's line count
  uint8_t* seq_next = nullptr;         // [ns] or null
};
// payload [1 + nk + ns + 1]; cnt (device [5] match / event counters, may be null) and caps (host
// [4]: gram, candidate, verified, event capacities) set the trailing overflow flag
void dp_pack(int64_t own_lines, const int64_t* freq, int nk, const int32_t* chain, int ns, int64_t* pack,
             uint64_t stream, bool dev, const int64_t* cnt = nullptr, const int64_t* caps = nullptr);
void dp_carry(const DpCarryArgs& A, uint64_t stream, bool dev);
}  // namespace lp

// ---- summary + top-k, streaming re-score (summarize.hip)
namespace lp {
struct SummIn {
  // events (level 0): score[i], pattern pat[i], global line = (line64 ? line64 : line32)[i] + *line_add
  const double* score;
  const int32_t* pat;
  const int32_t* line32;
  const int64_t* line64;
  const int64_t* line_add;   // device (host twin: host) scalar, may be null
  const int32_t* sev_of_pat; // [P] severity index 0..4
  // or rows [n][3] = (score, line, pattern) as float64 (merging top-k lists)
  const double* rows;
  // optional (events): every event packed as [global line int64 x n][score f64 x n][pattern i32 x n]
  void* ev_out = nullptr;
  // optional (events): device event count; n is then a capacity and the level-0 pass reads
  // min(n, *dn) events (ev_out packed at stride min(n, *dn))
  const int64_t* dn = nullptr;
};
// writes the k best rows (score desc, line asc, pattern asc; missing rows = (-inf, -1, -1)) and,
// from events, adds the pattern / severity histograms. Device: returns workspace bytes, runs only
// when ws_bytes suffices.
size_t summarize_dev(const SummIn& in, int64_t n, int k, int nsev, double* top_rows, unsigned long long* pat_hist,
                     unsigned long long* sev_hist, void* ws, size_t ws_bytes, uint64_t stream);
void summarize_host(const SummIn& in, int64_t n, int k, double* top_rows, int64_t* pat_hist, int64_t* sev_hist);
void rescore_dev(const int64_t* gl, const double* fac, int64_t n, int64_t N, const ScoreParams& S, double* out,
                 uint64_t stream);
void rescore_host(const int64_t* gl, const double* fac, int64_t n, int64_t N, const ScoreParams& S, double* out);
}  // namespace lp

// ---- post-match pipeline (lp_post.hip): hit CSR, events, frequency ranks, context features
namespace lp {
struct EvTables {
  const int64_t* prim_off;   // [R+1] patterns whose primary regex is r: prim_pats[prim_off[r]..]
  const int32_t* prim_pats;
  const int32_t* freq_key;   // [P] frequency key, -1 = pattern without id
  const int32_t* ctx_before; // [P] -1 = no context rules
  const int32_t* ctx_after;
  const int32_t* seg_lo; const int32_t* seg_hi; const int32_t* own_lo; const int32_t* own_hi;
  int nseg;
  int nkeys;
  int pbits;                 // bits of a pattern index
};

struct HitsArgs {
  const int64_t* cand;       // (regex << 32 | line): [0, pre_from) to DFA-verify, [pre_from, n) pre-verified
  int64_t n, pre_from;
  // device-count mode (dcount != null): cand[0, pre_from) and cand2[0, n - pre_from) are two
  // fixed-capacity regions whose used lengths are the device counters dcount[0] / dcount[1]
  // (the matchers' append counters: no host read between matching and the hit CSR)
  const int64_t* cand2 = nullptr;
  const unsigned long long* dcount = nullptr;
  int lbits, rbits, R;
  const uint8_t* text; const int64_t* ls; const int32_t* ll;
  DfaPool dfa;
  EvTables ev;
  // outputs (capacity n; hit_off R+1)
  int64_t* hits; int32_t* hit_line; int64_t* hit_off; int64_t* ev_cnt; int64_t* ev_end;
  int64_t* counters;         // [0] unique verified hits, [1] events
  bool cand_verified = false;  // small path: the caller ran cand_verify_all_dev already
};

struct EventsArgs {
  const int64_t* hits; int64_t nh;
  const int64_t* ev_cnt; const int64_t* ev_end;
  int64_t ne, L;
  int lbits;
  EvTables ev;
  const uint8_t* text; const int64_t* ls; const int32_t* ll;
  DfaPool dfa;
  int ctx_trans, ctx_acc;    // table extents of the 4 context DFAs (pool entries 0..3), for LDS staging
  // device-count mode (request path): [nh, ne] on the device; nh / ne above are then capacities
  // and a batch over them leaves the outputs unset (the caller re-runs with host counts)
  const int64_t* dcounts = nullptr;
  // device-count mode, bulk path (optional): receives the event count when the events fit ne, else
  // 0 -- the count every later kernel of the batch reads (event fields past it are unset)
  int64_t* ne_fit = nullptr;
  // outputs
  int32_t* ev_line; int32_t* ev_pat; int32_t* ev_seg; int64_t* ev_rank; int64_t* ev_fkey;
  int64_t* freq_counts;      // [nkeys]
  uint8_t* feat;             // [L] context features (nullptr: coverage only)
  int32_t* cov;              // [L] optional: window coverage out
  bool feat_ready = false;   // feat already holds every line's features (feat_all_dev): skip them
};

int bits_for(int64_t n);
// device versions return the workspace bytes they need; they only run when ws_bytes suffices
size_t hits_dev(const HitsArgs& A, void* ws, size_t ws_bytes, uint64_t stream);
// context features of EVERY line (k_feat_cov without a coverage filter): the request runner computes
// them on its side stream while the matchers run, so the event stage needs no feature pass
void feat_all_dev(int64_t L, const uint8_t* text, const int64_t* ls, const int32_t* ll, const DfaPool& P,
                  int ctx_trans, int ctx_acc, uint8_t* feat, uint64_t stream);
size_t events_dev(const EventsArgs& A, void* ws, size_t ws_bytes, uint64_t stream);

// A request's tail in one workgroup (lp_post.hip k_request_tail): hits_dev's and events_dev's small
// paths (device-count mode, features computed already), score_dev and publish_record_dev in one
// launch. The results layout is publish_record_dev's.
struct RequestTailOut {
  double* score;             // = (double*)out: the score column of the results buffer
  const uint8_t* out;        // results [score f64 x E | counts i64 x K1 | line | pattern | seg i32 x E]
  int64_t E;                 // the results' event capacity
  int K1;                    // max(nkeys, 1)
  const int64_t* cnt;        // device counters [gram, cand, ver, hits, events]
  int64_t* cnt_host;         // device views of the pinned host counters / results
  uint8_t* res_host;
  const int64_t* counts;     // the batch's per-key counts (results buffer) for the record
  int K;                     // frequency keys
  double now;
  FreqRing ring;
  RecordGate gate;
};
void request_tail_dev(const HitsArgs& HA, const EventsArgs& EA, const ScoreTables& T, const ScoreParams& S,
                      const FreqIn& F, const RequestTailOut& P, void* ws, size_t ws_bytes, uint64_t stream);
// capacities of the single-workgroup request path (events, lines): a batch within them can run
// the event stage in device-count mode
int64_t request_event_cap();
int64_t request_line_cap();
// n16 16-byte words from device-visible pinned host memory (host_dev) into device memory
// (request_io.hip)
void fetch_dev(const void* host_dev, void* dst, int64_t n16, uint64_t stream);
// device-count-mode results -> pinned host memory (request_io.hip): the 5 matcher/event counters
// and the results compacted to stride ne (cnt[4]) when ne <= E; both pointers device-visible
void publish_dev(const int64_t* cnt, const uint8_t* out, int64_t E, int K1, int64_t* cnt_host, uint8_t* res_host,
                 uint64_t stream);
// publish_dev + the batch's gated frequency record (k_freq_record) in one launch
void publish_record_dev(const int64_t* cnt, const uint8_t* out, int64_t E, int K1, int64_t* cnt_host,
                        uint8_t* res_host, const int64_t* counts, int K, double now, const FreqRing& R,
                        const RecordGate& G, uint64_t stream);
void blk_index_dev(const int64_t* ls, int64_t L, int64_t nblocks, int32_t* blk, uint64_t stream);
void hits_host(const HitsArgs& A);
void events_host(const EventsArgs& A);
void blk_index_host(const int64_t* ls, int64_t L, int64_t nblocks, int32_t* blk);
// host twin of feat_all_dev: context_feat of every line
void feat_all_host(int64_t L, const uint8_t* text, const int64_t* ls, const int32_t* ll, const DfaPool& P,
                   uint8_t* feat);
}  // namespace lp

// ---- coverage-gap report (gaps.hip): template signatures of the error lines no event explains
namespace lp {
struct GapSigArgs {
  const uint8_t* text;       // 16-byte aligned on the device
  int64_t tbytes;            // bytes of `text` that may be read (lines are clipped to it)
  const int64_t* ls; const int32_t* ll;
  int64_t L;
  // self-selecting (sel == null, all == false): line x is signed when gap_candidate(feat[x]) and it
  // is not covered (cov == null: nothing is covered)
  const uint8_t* feat = nullptr;   // [L] context features of every line
  const uint8_t* cov = nullptr;    // [L] or null
  // listed: sign exactly sel[0, nsel) (out slot i = sel[i]; a line outside [0, L) signs as empty);
  // all: sign every line (out slot x = line x)
  const int32_t* sel = nullptr;
  int64_t nsel = 0;
  bool all = false;
  // outputs: (line, signature bit pattern) pairs, the first `cap` of them; cnt[0] += candidates,
  // cnt[1] += selected lines (all of them: above cap the caller re-runs, as with scan_dev)
  int32_t* out_line; int64_t* out_sig;
  int64_t cap;
  unsigned long long* cnt;   // [2], zeroed by the caller
};
void gap_sig_dev(const GapSigArgs& A, uint64_t stream);
// appends in line order
void gap_sig_host(const GapSigArgs& A);
}  // namespace lp

// ---- signature group table (gap_table.hip): the grouping of the report across chunks and documents
#include "gap_table.h"
namespace lp {
struct GapRows {             // rows of a table, or the rows to put into one
  int64_t* sig; int64_t* count; int64_t* first;
  int32_t* docs; int32_t* last_doc;
};
// n pairs (sig[i], ord[i]) of document `doc` into the table; the caller keeps 2 * (used + n) <= cap,
// launches one document at a time and never a smaller document number than before. tile: pairs per
// block (256..2048, a multiple of 256), 0: chosen from n
void gap_fold_dev(const GapTab& T, const int64_t* sig, const int64_t* ord, int64_t n, int doc, uint64_t stream,
                  int tile = 0);
// after the fold of the same pairs: out[*cnt ...] = i for every pair whose ordinal is its group's
// smallest (out holds n entries; *cnt grows by the number appended)
void gap_winners_dev(const GapTab& T, const int64_t* sig, const int64_t* ord, int64_t n, int64_t* out,
                     unsigned long long* cnt, uint64_t stream);
// the occupied slots as rows, in no particular order: the first out_cap of them; *cnt += all of them
void gap_rows_dev(const GapTab& T, const GapRows& R, int64_t out_cap, unsigned long long* cnt, uint64_t stream);
// n rows of distinct signatures into a table that holds none of them (growth); used[0] is left to
// the caller, who knows it is n
void gap_reinsert_dev(const GapTab& T, const GapRows& R, int64_t n, uint64_t stream);
void gap_fold_host(const GapTab& T, const int64_t* sig, const int64_t* ord, int64_t n, int doc);
void gap_winners_host(const GapTab& T, const int64_t* sig, const int64_t* ord, int64_t n, int64_t* out,
                      unsigned long long* cnt);
void gap_rows_host(const GapTab& T, const GapRows& R, int64_t out_cap, unsigned long long* cnt);
void gap_reinsert_host(const GapTab& T, const GapRows& R, int64_t n);
}  // namespace lp

// ---- novelty report (novelty.hip): the lines whose template signature a baseline table does not hold
namespace lp {
struct NovelSigArgs {
  const uint8_t* text;       // 16-byte aligned on the device
  int64_t tbytes;            // bytes of `text` that may be read (lines are clipped to it)
  const int64_t* ls; const int32_t* ll;
  int64_t L;
  GapTab tab;                // the baseline: only read (key column and cap)
  const uint8_t* feat = nullptr;   // [L] context features of every line, or null: no candidates
  const uint8_t* evm = nullptr;    // [L] 1 where an event lies on the line, or null
  // outputs: every line x of [0, L) whose signature is not in `tab`, the first `cap` of them, as
  // (line, signature bit pattern, flag: bit0 gap_candidate(feat[x]), bit1 evm[x]);
  // cnt[0] += candidates among all lines, cnt[1] += novel lines (all of them: above cap the caller
  // re-runs, as with gap_sig_dev), cnt[2] += novel candidates
  int32_t* out_line; int64_t* out_sig; uint8_t* out_flag;
  int64_t cap;
  unsigned long long* cnt;   // [3], zeroed by the caller
};
// per_block: lines per block (rounded up to a multiple of 256, at most 2048), 0: chosen from L.
// GPU: the triples come in no particular order
void novel_sig_dev(const NovelSigArgs& A, uint64_t stream, int per_block = 0);
// appends in line order
void novel_sig_host(const NovelSigArgs& A);
// out[i] = 1 when the table holds sig[i] (the signature that equals the empty marker included)
void gap_contains_dev(const GapTab& T, const int64_t* sig, int64_t n, uint8_t* out, uint64_t stream);
void gap_contains_host(const GapTab& T, const int64_t* sig, int64_t n, uint8_t* out);
}  // namespace lp

// ---- lead-up report (leadup.hip): every line's signature, and the lines within W lines before an event
namespace lp {
struct LeadSigArgs {
  const uint8_t* text;       // 16-byte aligned on the device
  int64_t tbytes;            // bytes of `text` that may be read (lines are clipped to it)
  const int64_t* ls; const int32_t* ll;
  int64_t L;                 // at most 2^31 - 1
  const int32_t* ev = nullptr;     // [ne] the lines that carry an event: sorted, distinct; null when ne == 0
  int64_t ne = 0;
  int W;                     // 1 .. 4096: line x is in the lead-up iff some ev[j] has x < ev[j] <= x + W
  // outputs: sig[x] = signature bit pattern and lead[x] = 0 / 1 of every line; the lead-up lines
  // again as (line, signature) pairs, the first `cap` of them; cnt[0] += lead-up lines (all of
  // them: above cap the caller re-runs, as with novel_sig_dev)
  int64_t* sig; uint8_t* lead;
  int32_t* out_line; int64_t* out_sig;
  int64_t cap;
  unsigned long long* cnt;   // [1], zeroed by the caller
};
// per_block: lines per block (rounded up to a multiple of 256, at most 2048), 0: chosen from L.
// GPU: the pairs come in no particular order
void lead_sig_dev(const LeadSigArgs& A, uint64_t stream, int per_block = 0);
// appends in line order
void lead_sig_host(const LeadSigArgs& A);
}  // namespace lp

// ---- correlation report (correlate.hip): the id-like tokens of lines as (line, key) pairs
namespace lp {
struct KeyLinesArgs {
  const uint8_t* text;       // 16-byte aligned on the device
  int64_t tbytes;            // bytes of `text` that may be read (lines are clipped to it)
  const int64_t* ls; const int32_t* ll;
  int64_t nl;                // lines of ls / ll, at most 2^31 - 1
  const int32_t* sel = nullptr;    // [n] item i walks line sel[i] (0 <= sel[i] < nl); null: line i
  int64_t n;                 // items walked: nl without sel
  GapTab tab;                // tab.key null: every key is emitted; else only the keys it holds (only read)
  int min_len;               // 4 .. 64: bytes of a key token at least (key_core.h)
  // outputs: the keys of every walked line (its first 8 distinct ones, then the table's filter) as
  // (line number, key bit pattern) pairs, the first `cap` of them; hit[i] = 0 / 1: item i emitted
  // a pair; cnt[0] += pairs (all of them: above cap the caller re-runs, as with lead_sig_dev),
  // cnt[1] += items with at least one pair
  int32_t* out_line; int64_t* out_key;
  uint8_t* hit;
  int64_t cap;
  unsigned long long* cnt;   // [2], zeroed by the caller
};
// per_block: lines per block (rounded up to a multiple of 256, at most 2048), 0: chosen from n.
// GPU: the pairs come in no particular order
void line_keys_dev(const KeyLinesArgs& A, uint64_t stream, int per_block = 0);
// appends in item order, the keys of a line in byte order
void line_keys_host(const KeyLinesArgs& A);
}  // namespace lp

// ---- values report (values.hip): template signature and numeric fields of every line
namespace lp {
struct ValLinesArgs {
  const uint8_t* text;       // 16-byte aligned on the device
  int64_t tbytes;            // bytes of `text` that may be read (lines are clipped to it)
  const int64_t* ls; const int32_t* ll;
  int64_t nl;                // lines of ls / ll, at most 2^31 - 1: every one is walked
  // outputs: sig[i] = template signature of line i (gaps_core.h); the values of every line (of its
  // first 8 fields, val_core.h) as (line number, val_key(signature, field), value) triples, the
  // first `cap` of them; cnt[0] += triples (all of them: above cap the caller re-runs, as with
  // line_keys_dev), cnt[1] += lines with at least one value
  int64_t* sig;
  int32_t* out_line; int64_t* out_key; int32_t* out_val;
  int64_t cap;
  unsigned long long* cnt;   // [2], zeroed by the caller
};
// per_block: lines per block (rounded up to a multiple of 256, at most 2048), 0: chosen from nl.
// GPU: the triples come in no particular order
void line_vals_dev(const ValLinesArgs& A, uint64_t stream, int per_block = 0);
// appends in line order, the fields of a line in byte order
void line_vals_host(const ValLinesArgs& A);
}  // namespace lp

// ---- variants report (variants.hip): the value hashes of every line's fields, counts per (field, value)
#include "var_table.h"
namespace lp {
struct VarLinesArgs {
  const uint8_t* text;       // 16-byte aligned on the device
  int64_t tbytes;            // bytes of `text` that may be read (lines are clipped to it)
  const int64_t* ls; const int32_t* ll;
  int64_t nl;                // lines of ls / ll, at most 2^31 - 1: every one is walked
  // outputs: sig[i] = template signature of line i (gaps_core.h); the first 8 fields of every line
  // (var_core.h) as (line number, val_key(signature, field), hash of the token) triples, the first
  // `cap` of them; cnt[0] += triples (all of them: above cap the caller re-runs, as with
  // line_vals_dev), cnt[1] += lines with at least one field
  int64_t* sig;
  int32_t* out_line; int64_t* out_field; int64_t* out_value;
  int64_t cap;
  unsigned long long* cnt;   // [2], zeroed by the caller
};
// per_block: lines per block (rounded up to a multiple of 256, at most 2048), 0: chosen from nl.
// GPU: the triples come in no particular order
void line_vars_dev(const VarLinesArgs& A, uint64_t stream, int per_block = 0);
// appends in line order, the fields of a line in byte order
void line_vars_host(const VarLinesArgs& A);
struct VarRows {             // rows of a value table, or the rows to put into one
  int64_t* field; int64_t* value; int64_t* count; int64_t* first; int64_t* last;
};
// n triples (field[i], value[i], ord[i]: the global line number) into the table: per (field, value)
// the number of triples, the smallest and the largest ordinal. A triple whose field `skip` holds
// (a GapTab used as a set; key == nullptr: the empty set) is dropped. The caller keeps
// 2 * (used + n) <= cap. tile: triples per block (256..2048, a multiple of 256), 0: chosen from n
void var_fold_dev(const VarTab& T, const GapTab& skip, const int64_t* field, const int64_t* value, const int64_t* ord,
                  int64_t n, uint64_t stream, int tile = 0);
// the occupied slots as rows, in no particular order: the first out_cap of them; *cnt += all of them
void var_rows_dev(const VarTab& T, const VarRows& R, int64_t out_cap, unsigned long long* cnt, uint64_t stream);
// n rows of distinct (field, value) into a table that holds none of them (growth, purge); used[0] is
// left to the caller, who knows it is n
void var_reinsert_dev(const VarTab& T, const VarRows& R, int64_t n, uint64_t stream);
// out[*cnt ...] = i for every triple whose (field, value) the table holds with first == ord[i] (out
// holds n entries; *cnt grows by the number appended)
void var_winners_dev(const VarTab& T, const int64_t* field, const int64_t* value, const int64_t* ord, int64_t n,
                     int64_t* out, unsigned long long* cnt, uint64_t stream);
void var_fold_host(const VarTab& T, const GapTab& skip, const int64_t* field, const int64_t* value, const int64_t* ord,
                   int64_t n);
void var_rows_host(const VarTab& T, const VarRows& R, int64_t out_cap, unsigned long long* cnt);
void var_reinsert_host(const VarTab& T, const VarRows& R, int64_t n);
void var_winners_host(const VarTab& T, const int64_t* field, const int64_t* value, const int64_t* ord, int64_t n,
                      int64_t* out, unsigned long long* cnt);
}  // namespace lp

// ---- spans report (spans.hip): stamp, signature and sampled keys of every line; a span per key
#include "span_table.h"
namespace lp {
struct SpanLinesArgs {
  const uint8_t* text;       // 16-byte aligned on the device
  int64_t tbytes;            // bytes of `text` that may be read (lines are clipped to it)
  const int64_t* ls; const int32_t* ll;
  int64_t nl;                // lines of ls / ll, at most 2^31 - 1: every one is walked
  int min_len;               // KEY_MIN_LEN_LO .. KEY_MAX_LEN
  int shift;                 // 0..64: only the keys of this hash sample (span_sampled) are emitted
  // outputs: sig[i] / ts[i] = template signature and stamp (TS_NONE: none) of line i, what
  // line_stamps_dev writes; the sampled ones of every line's first 8 distinct keys (key_core.h) as
  // (line number, key, place of the token: key_pos_pack) triples, the first `cap` of them;
  // cnt[0] += triples (all of them: above cap the caller re-runs, as with line_keys_dev),
  // cnt[1] += lines with at least one triple; lvl (optional): lvl[m] += the lines with a triple whose
  // deepest key has level m (span_level) -- the lines that still hold a key under every shift <= m
  int64_t* sig; int64_t* ts;
  int32_t* out_line; int64_t* out_key; int32_t* out_tok;
  int64_t cap;
  unsigned long long* cnt;   // [2], zeroed by the caller
  unsigned long long* lvl;   // [SPAN_LEVELS] or null
};
// per_block: lines per block (rounded up to a multiple of 256, at most 2048), 0: chosen from nl.
// GPU: the triples come in no particular order
void span_keys_dev(const SpanLinesArgs& A, uint64_t stream, int per_block = 0);
// appends in line order, the keys of a line in byte order
void span_keys_host(const SpanLinesArgs& A);
struct SpanPairs {           // the triples of one span_keys call with what the table needs of its lines
  const int32_t* line; const int64_t* key; const int32_t* tok;
  int64_t n;
  const int64_t* sig;        // [nl] signatures of the piece's lines
  const int64_t* eff;        // [nl] effective times (TS_NONE: none)
  int64_t nl;
  const uint8_t* text; int64_t tbytes;   // the piece's text, still resident: the tokens are cut from it
  const int64_t* ls;         // [nl] line starts in `text`
  int64_t line_base;         // global number of the piece's line 0
};
// fold: count, first / last line and smallest / largest effective time per key. A pair whose line is
// outside [0, nl) is counted in used[1]. The caller keeps 2 * (used + n) <= cap.
void span_fold_dev(const SpanTab& T, const SpanPairs& X, uint64_t stream);
// ends, after the fold of the SAME pairs on the same stream (first / last are final only then):
// opens, toklen and tok from the pair that holds the span's first line, closes from the one that
// holds its last
void span_ends_dev(const SpanTab& T, const SpanPairs& X, uint64_t stream);
// the occupied slots whose key is in sample `shift` (span_sampled; 0: all) as rows, in no particular
// order: the first out_cap of them; *cnt += all of them
void span_rows_dev(const SpanTab& T, const SpanRows& R, int64_t out_cap, unsigned long long* cnt, uint64_t stream,
                   int shift = 0);
// n rows of distinct keys into a table that holds none of them (growth, purge); used[0] is left to
// the caller, who knows it is n
void span_reinsert_dev(const SpanTab& T, const SpanRows& R, int64_t n, uint64_t stream);
void span_fold_host(const SpanTab& T, const SpanPairs& X);
void span_ends_host(const SpanTab& T, const SpanPairs& X);
void span_rows_host(const SpanTab& T, const SpanRows& R, int64_t out_cap, unsigned long long* cnt, int shift = 0);
void span_reinsert_host(const SpanTab& T, const SpanRows& R, int64_t n);
}  // namespace lp

// ---- log timeline (timeline.hip): the timestamp of every line, counts per time bucket
namespace lp {
// out[i] = epoch milliseconds (UTC) of the stamp at the head of line i, or TS_NONE = INT64_MIN
// (ts_core.h line_ts_at); text: 16-byte aligned on the device, tbytes: bytes of it that may be read
void ts_parse_dev(const uint8_t* text, int64_t tbytes, const int64_t* ls, const int32_t* ll, int64_t L, int64_t* out,
                  uint64_t stream);
void ts_parse_host(const uint8_t* text, int64_t tbytes, const int64_t* ls, const int32_t* ll, int64_t L, int64_t* out);
// forward fill and out-of-order count over the stamps ts[0, L) in line order: eff[i] = the stamp
// of the nearest stamped line at or before i, else carry_last (the same of the earlier chunks, or
// TS_NONE); *ooo += the stamped lines whose stamp is below the largest stamp before them
// (carry_top: the largest of the earlier chunks, or TS_NONE). tmp: tl_fill_tmp_words(L) words.
void tl_fill_dev(const int64_t* ts, int64_t L, int64_t carry_last, int64_t carry_top, int64_t* eff,
                 unsigned long long* ooo, int64_t* tmp, uint64_t stream);
int64_t tl_fill_tmp_words(int64_t L);
void tl_fill_host(const int64_t* ts, int64_t L, int64_t carry_last, int64_t carry_top, int64_t* eff,
                  unsigned long long* ooo);
struct TlHistArgs {
  const int64_t* eff;        // [L] effective time of every line, TS_NONE: undated
  const uint8_t* feat;       // [L] context features of every line
  int64_t L;
  const int32_t* ev_line;    // [E] the events' lines (an event outside [0, L) is not counted)
  const int32_t* ev_pat;     // [E] their patterns
  int64_t E;
  const int32_t* sev_index;  // [P] severity number of every pattern
  int64_t P;
  int S;                     // distinct severities
  int64_t t0, W, nb;         // bucket b covers [t0 + b * W, t0 + (b + 1) * W) milliseconds
  int64_t* hist;             // [nb][3 + S], added to: lines, error lines, events, one column per severity
};
void tl_hist_dev(const TlHistArgs& A, uint64_t stream);
void tl_hist_host(const TlHistArgs& A);
}  // namespace lp

// ---- trends report (trends.hip): stamp and signature of every line, counts per (signature, time bucket)
#include "cell_table.h"
namespace lp {
struct LineStampsArgs {
  const uint8_t* text;       // 16-byte aligned on the device
  int64_t tbytes;            // bytes of `text` that may be read (lines are clipped to it)
  const int64_t* ls; const int32_t* ll;
  int64_t nl;                // lines of ls / ll, at most 2^31 - 1: every one is walked
  // outputs: sig[i] = template signature of line i (gaps_core.h), ts[i] = epoch milliseconds of its
  // stamp or TS_NONE (ts_core.h)
  int64_t* sig; int64_t* ts;
};
// per_block: lines per block (rounded up to a multiple of 256, at most 2048), 0: chosen from nl
void line_stamps_dev(const LineStampsArgs& A, uint64_t stream, int per_block = 0);
void line_stamps_host(const LineStampsArgs& A);
struct CellRows {            // rows of a cell table, or the rows to put into one
  int64_t* sig; int64_t* bucket; int64_t* count; int64_t* first;
};
// n consecutive lines, line i with the signature sig[i], the effective time eff[i] (TS_NONE: undated,
// the cell of the bucket CT_UNDATED) and the global number line_base + i, into the table: per cell
// (sig, floor(eff / W)) the number of lines and the smallest line. The caller keeps
// 2 * (used + n) <= cap. tile: lines per block (256..2048, a multiple of 256), 0: chosen from n
void cell_fold_dev(const CellTab& T, const int64_t* sig, const int64_t* eff, int64_t n, int64_t line_base, int64_t W,
                   uint64_t stream, int tile = 0);
// the occupied slots as rows, in no particular order: the first out_cap of them; *cnt += all of them
void cell_rows_dev(const CellTab& T, const CellRows& R, int64_t out_cap, unsigned long long* cnt, uint64_t stream);
// n rows of distinct cells into a table that holds none of them (growth); used[0] is left to the
// caller, who knows it is n
void cell_reinsert_dev(const CellTab& T, const CellRows& R, int64_t n, uint64_t stream);
void cell_fold_host(const CellTab& T, const int64_t* sig, const int64_t* eff, int64_t n, int64_t line_base, int64_t W);
void cell_rows_host(const CellTab& T, const CellRows& R, int64_t out_cap, unsigned long long* cnt);
void cell_reinsert_host(const CellTab& T, const CellRows& R, int64_t n);
}  // namespace lp

// ---- pauses report (pauses.hip): the steps between the stamped lines of a log, the long ones as rows
namespace lp {
constexpr int PS_BUCKETS = 64;      // interval histogram: bucket = bit length of the step (0 for 0)
// columns of the statistics: sums are added to, the smallest / largest stamp lowered / raised
// (start: 0, 0, 0, INT64_MAX, INT64_MIN)
enum { PS_STAMPED = 0, PS_BACKWARD = 1, PS_PAUSED_MS = 2, PS_MIN_TS = 3, PS_MAX_TS = 4, PS_STATS = 5 };
struct PauseRows {           // one row per pause, in line order
  int64_t* to_line; int64_t* from_line;      // global line numbers
  int64_t* ms;                               // the step
  int64_t* from_sig; int64_t* to_sig;        // the two lines' template signatures
};
struct PauseArgs {
  const int64_t* ts;         // [L] stamp of every line or TS_NONE, within +-2^61
  const int64_t* sig;        // [L] template signature of every line
  int64_t L;
  int64_t line_base;         // global number of line 0
  int64_t min_ms;            // >= 1: a step >= min_ms is a pause
  // the last stamped line of the earlier runs: its stamp (TS_NONE: none), its global line
  // (< line_base) and its signature
  int64_t carry_ts, carry_line, carry_sig;
  int64_t* tmp;              // device: pause_tmp_words(L) words, written by pause_count_dev, read by pause_emit_dev
  // pause_count: [0] the pauses of this run, [1..3] stamp, line, signature of the last stamped
  // line so far (TS_NONE, -1, 0: still none)
  int64_t* head;
  // pause_emit: the first `cap` rows; stats[PS_STATS] and hist[PS_BUCKETS] are added to
  PauseRows rows;
  int64_t cap;
  int64_t* stats;
  int64_t* hist;
};
int64_t pause_tmp_words(int64_t L);
// two calls per run, so that the caller can size the rows from head[0] in between; L = 0 launches nothing
void pause_count_dev(const PauseArgs& A, uint64_t stream);
void pause_emit_dev(const PauseArgs& A, uint64_t stream);
void pause_count_host(const PauseArgs& A);
void pause_emit_host(const PauseArgs& A);
}  // namespace lp

// ---- cadence report (cadence.hip): per stamped line the beat since the previous stamped line of its
// template; one row per template, joined across tiles and runs
namespace lp {
// columns of a row: consecutive stamped occurrences of one signature. lines = beats + backward + 1;
// sum / min / max speak of the forward beats (min INT64_MAX, max -1, max_from / max_to -1: none);
// max_from / max_to: the lines of the first largest beat, max_to_ts the stamp of its to-line
enum { CD_SIG = 0, CD_LINES = 1, CD_BEATS = 2, CD_BACKWARD = 3, CD_SUM = 4, CD_MIN = 5, CD_MAX = 6, CD_MAX_FROM = 7,
       CD_MAX_TO = 8, CD_FIRST_LINE = 9, CD_LAST_LINE = 10, CD_LAST_TS = 11, CD_FIRST_TS = 12, CD_MAX_TO_TS = 13,
       CD_COLS = 14 };
struct CadenceTileArgs {
  const int64_t* ts;         // [L] stamp of every line or TS_NONE, within +-2^61
  const int64_t* sig;        // [L] template signature of every line
  int64_t L;
  int64_t line_base;         // global number of line 0
  // beat[i]: the line's beat inside its tile of 2,048 lines, TS_NONE for an unstamped line and for
  // the first stamped line of its signature in the tile; bkt[i]: bit length of a beat >= 0, else TS_NONE
  int64_t* beat; int64_t* bkt;
  // one row per (tile, signature), CD_COLS columns of `cap` entries each: the first `cap` of them;
  // *cnt += all of them (above cap the caller reruns). GPU: in no particular order
  int64_t* rows;
  int64_t cap;
  unsigned long long* cnt;
};
struct CadenceLinkArgs {
  const int64_t* in;         // CD_COLS columns of R entries: rows sorted by (signature, first line)
  int64_t R;
  int64_t* out;              // CD_COLS columns of `cap` entries: one row per signature, sorted by signature
  int64_t cap;
  int64_t* head;             // [0] the output rows (all of them)
  int64_t* tmp;              // device: cadence_link_tmp_words(R) words
  // the run's lines: a row that follows one of its signature writes the beat of its first line
  // when that line lies in [line_base, line_base + L)
  int64_t line_base, L;
  int64_t* beat; int64_t* bkt;
};
int64_t cadence_link_tmp_words(int64_t R);
void cadence_tile_dev(const CadenceTileArgs& A, uint64_t stream);
void cadence_link_dev(const CadenceLinkArgs& A, uint64_t stream);
// rows per tile in the order of their first lines
void cadence_tile_host(const CadenceTileArgs& A);
void cadence_link_host(const CadenceLinkArgs& A);
}  // namespace lp

// ---- trace report (traces.hip): stack traces as runs of frame / cause lines, one row per trace
#include "trace_core.h"
namespace lp {
// cls[i] = class of line i (TR_OTHER / TR_FRAME / TR_MORE / TR_CAUSE), elem[i] = what it contributes
// to its trace's signature (0 for OTHER and MORE); text: 16-byte aligned on the device
void trace_class_dev(const uint8_t* text, int64_t tbytes, const int64_t* ls, const int32_t* ll, int64_t L, uint8_t* cls,
                     uint64_t* elem, uint64_t stream);
void trace_class_host(const uint8_t* text, int64_t tbytes, const int64_t* ls, const int32_t* ll, int64_t L, uint8_t* cls,
                      uint64_t* elem);
struct TraceRunArgs {
  const uint8_t* cls;        // [L]
  const uint64_t* elem;      // [L]
  const uint8_t* evm = nullptr;   // [L] 1 where an event lies on the line, or null
  int64_t L;                 // 1 .. 2^31 - 1
  TrCarry in;                // what the previous piece left (line numbers count from this piece's first line)
  bool last;                 // no later piece follows: a run that reaches the last line ends there
  // outputs: one row per trace that ends in this piece, the first `cap` of them, as TR_COLS columns
  // of `cap` entries each (start line, signature, lines, frames, causes, flags, first FRAME line,
  // last CAUSE line; line numbers count from this piece's first line and are negative for a run
  // that came in); cnt[0] += the traces (all of them: above cap the caller re-runs);
  // carry_out[TR_CARRY_WORDS]: what this piece leaves, counted from the next piece's first line
  int64_t* out;
  int64_t cap;
  unsigned long long* cnt;   // [1], zeroed by the caller
  int64_t* carry_out;
};
int trace_tile();            // lines per block of the three scan launches
int64_t trace_runs_tmp_bytes(int64_t L);
// GPU: the rows come in no particular order. tmp: trace_runs_tmp_bytes(L) bytes, 8-byte aligned
void trace_runs_dev(const TraceRunArgs& A, void* tmp, uint64_t stream);
// appends in line order
void trace_runs_host(const TraceRunArgs& A);
}  // namespace lp
