// Native request runner (see request.h).
#include "runtime/request.h"

#include <cstdio>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

namespace lp {

namespace {

constexpr int64_t kNlTile = 16384;   // ops/kernels.py NL_TILE / TEXT_PAD
constexpr int64_t kTextPad = 64;
constexpr int kBlkShift = 12;        // LINE_BLK_SHIFT
constexpr size_t kFetchMaxBytes = size_t(4) << 20;   // k_fetch up to this upload size

void check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP error in request runner (") + what + "): " + hipGetErrorString(e));
}

int64_t padded_len(int64_t n) { return ((std::max<int64_t>(n, 1) + kNlTile - 1) / kNlTile) * kNlTile + kTextPad; }

size_t up256(size_t n) { return (n + 255) & ~size_t(255); }

// pinned host memory kernels write into (k_publish): fine-grained, so the GPU's stores go to
// host memory and are visible once the stream has synchronised
constexpr unsigned kCoherentHost = hipHostMallocMapped | hipHostMallocCoherent;

// a device or pinned buffer that only grows (between runs, when nothing in flight uses it)
template <bool Pinned>
void grow(uint8_t*& p, size_t& cap, size_t need, unsigned host_flags = hipHostMallocDefault) {
  if (need <= cap) return;
  const size_t n = std::max(need + need / 4, size_t(1) << 20);
  if (p) check(Pinned ? hipHostFree(p) : hipFree(p), "free");
  p = nullptr;
  cap = 0;
  check(Pinned ? hipHostMalloc(reinterpret_cast<void**>(&p), n, host_flags)
               : hipMalloc(reinterpret_cast<void**>(&p), n), "alloc");
  cap = n;
}

template <typename T>
T* device_view(T* host) {
  void* d = nullptr;
  check(hipHostGetDevicePointer(&d, host, 0), "host device pointer");
  return static_cast<T*>(d);
}

// The inputs of a request as ONE region: the padded text, then the line index, the segments, the
// matcher counters (zeroed) and the sequence carry (zeroed), each 256-aligned. The single-copy host
// staging behind the text, upload_bytes() and the head of the workspace carve all use these offsets.
struct UploadLayout {
  size_t tsize;                        // padded text
  size_t o_ls, o_ll, o_seg, o_cnt, o_seq;
  size_t s_hi, s_g0, s_n;              // inside the segment block (lo first)
  size_t seg_bytes, nseq1;
  size_t total;                        // whole 16-byte words
};

UploadLayout upload_layout(int64_t nbytes, int64_t L, int D, int nseq) {
  const size_t L1 = (size_t)std::max<int64_t>(L, 1);
  UploadLayout u;
  u.tsize = (size_t)padded_len(nbytes);
  u.s_hi = up256(4 * (size_t)D);
  u.s_g0 = 2 * u.s_hi;
  u.s_n = u.s_g0 + up256(8 * (size_t)D);
  u.seg_bytes = u.s_n + up256(8 * (size_t)D);
  u.nseq1 = (size_t)std::max(nseq, 1);
  u.o_ls = up256(u.tsize);
  u.o_ll = u.o_ls + up256(8 * L1);
  u.o_seg = u.o_ll + up256(4 * L1);
  u.o_cnt = u.o_seg + up256(u.seg_bytes);
  u.o_seq = u.o_cnt + up256(8 * sizeof(int64_t));
  u.total = (u.o_seq + u.nseq1 + 15) & ~size_t(15);
  return u;
}

// views of a results buffer of event capacity E (layout: request.h run())
struct Results {
  double* score;
  int64_t* counts;
  int32_t *line, *pat, *seg;
};

Results results_view(uint8_t* out, int64_t E, int K1) {
  Results v;
  v.score = reinterpret_cast<double*>(out);
  v.counts = reinterpret_cast<int64_t*>(out + 8 * (size_t)E);
  v.line = reinterpret_cast<int32_t*>(out + 8 * (size_t)E + 8 * (size_t)K1);
  v.pat = v.line + E;
  v.seg = v.pat + E;
  return v;
}

size_t results_bytes(int64_t E, int K1) { return 20 * (size_t)E + 8 * (size_t)K1; }

}  // namespace

struct RequestRunner::Run {
  // arguments of run()
  uint8_t* host_text;
  int64_t nbytes;
  const int64_t* starts;
  const int32_t* lens;
  int64_t L;
  int D;
  const FreqRing& ring;
  double evict_before, now;
  uint64_t stream;
  Turn* turn;
  int64_t seq;
  const int64_t* inj;
  int64_t ninj;
  HostWindow* hw;
  hipStream_t st;
  // per run
  UploadLayout up;
  bool one_copy = false;
  const uint8_t* text_dev_src = nullptr;   // the stage buffer as the device sees it (k_fetch), or null
  bool text_up = false;                    // the text is on its way already (prefetch_text)
  int64_t nblk = 0;
  int lbits = 0, rbits = 0, K1 = 1;
  int64_t ecap = 0;                        // event capacity of the single-workgroup paths
  bool in_window = false;                  // this batch's eviction has been queued
  int64_t hw_seq = -1;                     // host window: the section's ticket (-1: not inside)
  double hw_now = 0.0;
  // per attempt
  int64_t cap_g = 0, cap_c = 0, cap_v = 0, n = 0;
  bool fast = false;                       // device-count mode
  bool feat_ready = false;                 // every line's features computed on the side stream
  EvTables ev;
  // carved from the workspace (carve / carve_events): the inputs in the upload's layout ...
  uint8_t* text = nullptr;
  int64_t* ls = nullptr;
  int32_t* ll = nullptr;
  int32_t *dlo = nullptr, *dhi = nullptr;
  int64_t *dg0 = nullptr, *dn = nullptr;
  int64_t* cnt = nullptr;
  uint8_t* seq_carry = nullptr;
  // ... the matchers' and the hit pipeline's buffers ...
  int32_t* blk = nullptr;
  int64_t *gh = nullptr, *cand = nullptr, *ver = nullptr, *inj_dev = nullptr;
  int64_t *hits = nullptr, *hit_off = nullptr, *ev_cnt = nullptr, *ev_end = nullptr;
  int32_t* hit_line = nullptr;
  // ... and the event stage's: results `out`, frequency ranks, context features
  uint8_t *out = nullptr, *feat = nullptr;
  int64_t *ev_rank = nullptr, *ev_fkey = nullptr;

  unsigned long long* c0() const { return reinterpret_cast<unsigned long long*>(cnt); }
  RecordGate gate() const {
    RecordGate G;
    G.cnt = cnt;
    G.cap[0] = cap_g; G.cap[1] = cap_c; G.cap[2] = cap_v; G.cap[3] = ecap;
    return G;
  }
  Results results(int64_t E) const { return results_view(out, E, K1); }

  // hit CSR + event counts: the pipeline reads the matchers' device counters itself
  HitsArgs hits_args(const RequestStatic& S, bool verified) const {
    HitsArgs A;
    A.cand = cand; A.n = n; A.pre_from = cap_c;
    A.cand2 = ver; A.dcount = c0() + 1;
    A.lbits = lbits; A.rbits = rbits; A.R = S.R;
    A.text = text; A.ls = ls; A.ll = ll; A.dfa = S.dfa; A.ev = ev;
    A.hits = hits; A.hit_line = hit_line; A.hit_off = hit_off; A.ev_cnt = ev_cnt; A.ev_end = ev_end;
    A.counters = cnt + 3;
    A.cand_verified = verified;
    return A;
  }
  // events, context features, frequency ranks into the results buffer of capacity E;
  // `dcnt` = device [nh, ne] (device-count mode, nh_cap / E = capacities) or null (counts read back)
  EventsArgs events_args(const RequestStatic& S, int64_t E, int64_t nh_cap, const int64_t* dcnt) const {
    const Results v = results(E);
    EventsArgs A;
    A.ctx_trans = S.ctx_trans; A.ctx_acc = S.ctx_acc;
    A.hits = (nh_cap || dcnt) ? hits : nullptr; A.nh = nh_cap; A.ev_cnt = ev_cnt; A.ev_end = ev_end; A.ne = E; A.L = L;
    A.lbits = lbits; A.ev = ev; A.text = text; A.ls = ls; A.ll = ll; A.dfa = S.dfa;
    A.ev_line = v.line; A.ev_pat = v.pat; A.ev_seg = v.seg; A.ev_rank = ev_rank; A.ev_fkey = ev_fkey;
    A.freq_counts = v.counts; A.feat = feat; A.cov = nullptr; A.dcounts = dcnt;
    A.feat_ready = feat_ready;
    return A;
  }
  // the per-pattern tables with this run's batch fields
  ScoreTables score_tables(const RequestStatic& S) const {
    ScoreTables T = S.st;
    T.seq_carry = seq_carry;
    T.hit_off = hit_off; T.hit_line = hit_line; T.feat = feat;
    T.seg_lo = dlo; T.seg_hi = dhi; T.seg_own_lo = dlo; T.seg_g0 = dg0; T.seg_n = dn;
    return T;
  }
  // what the event stage expects zeroed and the upload did not bring
  void zero_event_inputs(const RequestStatic& S, int64_t E) const {
    if (S.nkeys == 0) check(hipMemsetAsync(results(E).counts, 0, 8, st), "counts");
    if (L == 0) check(hipMemsetAsync(feat, 0, 1, st), "feat");
    if (!one_copy) check(hipMemsetAsync(seq_carry, 0, up.nseq1, st), "seq carry");
  }
};

RequestRunner::RequestRunner(const RequestStatic& S) : S_(S) {
  check(hipSetDevice(S_.device), "set device");
  check(hipHostMalloc(reinterpret_cast<void**>(&cnt_host_), 8 * sizeof(int64_t), kCoherentHost), "pinned counters");
  cnt_host_dev_ = device_view(cnt_host_);
  // literal-free scans + context features beside the literal chain
  check(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking), "side stream");
  check(hipEventCreateWithFlags(&fork_, hipEventDisableTiming), "fork event");
  check(hipEventCreateWithFlags(&join_, hipEventDisableTiming), "join event");
}

RequestRunner::~RequestRunner() {
  if (fork_) (void)hipEventDestroy(fork_);
  if (join_) (void)hipEventDestroy(join_);
  if (side_) (void)hipStreamDestroy(side_);
  if (carry_host_) (void)hipHostFree(carry_host_);
  if (ws_) (void)hipFree(ws_);
  if (post_ws_) (void)hipFree(post_ws_);
  if (up_host_) (void)hipHostFree(up_host_);
  if (inj_host_) (void)hipHostFree(inj_host_);
  if (res_host_) (void)hipHostFree(res_host_);
  if (cnt_host_) (void)hipHostFree(cnt_host_);
}

uint8_t* RequestRunner::dev(size_t bytes) {
  uint8_t* p = ws_ ? ws_ + ws_used_ : nullptr;
  ws_used_ += up256(bytes);
  return p;
}

void RequestRunner::ensure_results(size_t bytes) {
  if (bytes <= res_cap_) return;
  grow<true>(res_host_, res_cap_, bytes, kCoherentHost);
  res_host_dev_ = device_view(res_host_);
}

int64_t RequestRunner::upload_bytes(int64_t nbytes, int64_t L, int D) const {
  return (int64_t)upload_layout(nbytes, L, D, S_.nseq).total;
}

bool RequestRunner::map_fetch(uint8_t* host_text, int64_t host_cap) {
  if (host_text != fetch_host_ || host_cap != fetch_cap_) {
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, host_text, 0) != hipSuccess) {
      (void)hipGetLastError();
      d = nullptr;
    }
    fetch_host_ = host_text;
    fetch_cap_ = host_cap;
    fetch_dev_ = static_cast<uint8_t*>(d);
  }
  return fetch_dev_ != nullptr;
}

int64_t RequestRunner::prefetch_text(uint8_t* host_text, int64_t nbytes, int64_t host_cap, uint64_t stream) {
  pre_host_ = nullptr;
  pre_n_ = -1;
  pre_token_ = 0;
  const int64_t tsize = padded_len(nbytes);
  if (!ws_ || (size_t)tsize > ws_cap_ || host_cap < tsize || (size_t)tsize > kFetchMaxBytes ||
      ((uintptr_t)host_text & 15) != 0)
    return 0;
  check(hipSetDevice(S_.device), "set device");
  if (!map_fetch(host_text, host_cap)) return 0;
  std::memset(host_text + nbytes, 0, (size_t)(tsize - nbytes));       // vector loads past the end
  fetch_dev(fetch_dev_, ws_, tsize / 16, stream);                     // the text is the carve's first region
  pre_host_ = host_text;
  pre_n_ = nbytes;
  pre_ws_ = ws_;
  pre_token_ = ++pre_next_;
  return pre_token_;
}

// Inputs. Single-copy layout (when host_cap allows): the line index, the segments, zeroed
// matcher counters and a zeroed sequence carry sit behind the padded text at the offsets the
// workspace carve gives them, so ONE H2D moves them all (each extra copy of a request
// cost ~8 us of DMA setup plus ~8 us of queue gap, and the counter memset another fill).
void RequestRunner::stage_inputs(Run& r, const int32_t* seg_lo, const int32_t* seg_hi, const int64_t* seg_g0,
                                 const int64_t* seg_n, int64_t host_cap, int64_t pre_token) {
  const UploadLayout& u = r.up;
  uint8_t* host_text = r.host_text;
  std::memset(host_text + r.nbytes, 0, u.tsize - (size_t)r.nbytes);   // vector loads past the end
  r.one_copy = host_cap >= (int64_t)u.total;
  // ... read by a kernel from the pinned buffer itself when the runtime maps it for the device
  // (request-sized uploads only: a multi-MB batch moves faster on the SDMA engine, ~50 vs ~37 GB/s)
  if (r.one_copy && u.total <= kFetchMaxBytes && ((uintptr_t)host_text & 15) == 0) {
    map_fetch(host_text, host_cap);
    r.text_dev_src = fetch_dev_;
  }
  // the text already on its way (prefetch_text, same buffer and length): upload what follows it
  r.text_up = pre_token > 0 && pre_token == pre_token_ && pre_host_ == host_text && pre_n_ == r.nbytes;
  pre_host_ = nullptr;
  pre_n_ = -1;
  pre_token_ = 0;
  uint8_t* segh;
  if (r.one_copy) {
    if (r.L > 0) {
      std::memcpy(host_text + u.o_ls, r.starts, 8 * (size_t)r.L);
      std::memcpy(host_text + u.o_ll, r.lens, 4 * (size_t)r.L);
    }
    std::memset(host_text + u.o_cnt, 0, 8 * sizeof(int64_t));
    std::memset(host_text + u.o_seq, 0, u.nseq1);
    segh = host_text + u.o_seg;
  } else {
    grow<true>(up_host_, up_cap_, u.seg_bytes);
    segh = up_host_;
  }
  std::memcpy(segh, seg_lo, 4 * (size_t)r.D);
  std::memcpy(segh + u.s_hi, seg_hi, 4 * (size_t)r.D);
  std::memcpy(segh + u.s_g0, seg_g0, 8 * (size_t)r.D);
  std::memcpy(segh + u.s_n, seg_n, 8 * (size_t)r.D);
}

void RequestRunner::size_attempt(Run& r, int attempt) const {
  r.cap_g = (int64_t)((double)r.L * rate_gram_ * 1.25) + 512;
  r.cap_c = (int64_t)((double)r.L * rate_cand_ * 1.25) + 512;
  r.cap_v = (int64_t)((double)r.L * rate_ver_ * 1.25) + 512 + r.ninj;
  r.n = r.cap_c + r.cap_v;
  // device-count mode: a request on the single-workgroup paths runs matching, CSR, events,
  // score and the (gated) frequency record without the mid-batch host read
  r.fast = S_.device_counts && attempt == 0 && r.n <= r.ecap && r.L <= request_line_cap();
}

// Every buffer of an attempt, in one place: with no workspace yet it only measures (ws_used_),
// and after the workspace has moved it is simply run again (same sizes, same offsets).
void RequestRunner::carve(Run& r) {
  const UploadLayout& u = r.up;
  ws_used_ = 0;
  uint8_t* in = dev(u.total);            // the inputs, in the single-copy host layout
  uint8_t* segs = in + u.o_seg;
  r.text = in;
  r.ls = reinterpret_cast<int64_t*>(in + u.o_ls);
  r.ll = reinterpret_cast<int32_t*>(in + u.o_ll);
  r.dlo = reinterpret_cast<int32_t*>(segs);
  r.dhi = reinterpret_cast<int32_t*>(segs + u.s_hi);
  r.dg0 = reinterpret_cast<int64_t*>(segs + u.s_g0);
  r.dn = reinterpret_cast<int64_t*>(segs + u.s_n);
  r.cnt = reinterpret_cast<int64_t*>(in + u.o_cnt);
  r.seq_carry = in + u.o_seq;
  r.blk = reinterpret_cast<int32_t*>(dev(4 * (size_t)r.nblk));
  // the upload ends before the next buffer begins
  if (ws_ && in + u.total > reinterpret_cast<uint8_t*>(r.blk))
    throw std::runtime_error("request runner: upload layout mismatch");
  r.gh = reinterpret_cast<int64_t*>(dev(8 * (size_t)r.cap_g));
  r.cand = reinterpret_cast<int64_t*>(dev(8 * (size_t)r.cap_c));
  r.ver = reinterpret_cast<int64_t*>(dev(8 * (size_t)r.cap_v));
  r.hits = reinterpret_cast<int64_t*>(dev(8 * (size_t)r.n));
  r.hit_line = reinterpret_cast<int32_t*>(dev(4 * (size_t)r.n));
  r.hit_off = reinterpret_cast<int64_t*>(dev(8 * (size_t)(S_.R + 1)));
  r.ev_cnt = reinterpret_cast<int64_t*>(dev(8 * (size_t)r.n));
  r.ev_end = reinterpret_cast<int64_t*>(dev(8 * (size_t)r.n));
  r.inj_dev = r.ninj > 0 ? reinterpret_cast<int64_t*>(dev(8 * (size_t)r.ninj)) : nullptr;
  if (r.fast) carve_events(r, r.ecap);
  r.ev.seg_lo = r.dlo;
  r.ev.seg_hi = r.dhi;
  r.ev.own_lo = r.dlo;
  r.ev.own_hi = r.dhi;
  r.ev.nseg = r.D;
}

// event-stage buffers (results layout: [score f64 x E | counts i64 x K1 | line | pattern | seg i32 x E])
void RequestRunner::carve_events(Run& r, int64_t E) {
  r.out = dev(results_bytes(E, r.K1));
  r.ev_rank = reinterpret_cast<int64_t*>(dev(8 * (size_t)std::max<int64_t>(E, 1)));
  r.ev_fkey = reinterpret_cast<int64_t*>(dev(8 * (size_t)std::max<int64_t>(E, 1)));
  r.feat = dev((size_t)std::max<int64_t>(r.L, 1));
}

// inputs: packed text, line index, segments (all pinned -> async)
void RequestRunner::upload(Run& r, int attempt) {
  const UploadLayout& u = r.up;
  if (r.text_up && (ws_ != pre_ws_ || r.text != ws_)) r.text_up = false;   // (the workspace moved: all again)
  if (r.one_copy && r.text_dev_src && r.text_up && attempt == 0) {
    const size_t o_rest = u.o_ls;              // 256-aligned: the index, segments, counters, carry
    fetch_dev(r.text_dev_src + o_rest, r.text + o_rest, (int64_t)((u.total - o_rest) / 16), r.stream);
  } else if (r.one_copy && r.text_dev_src) {
    fetch_dev(r.text_dev_src, r.text, (int64_t)(u.total / 16), r.stream);
  } else if (r.one_copy) {
    check(hipMemcpyAsync(r.text, r.host_text, u.total, hipMemcpyHostToDevice, r.st), "inputs H2D");
  } else {
    check(hipMemcpyAsync(r.text, r.host_text, u.tsize, hipMemcpyHostToDevice, r.st), "text H2D");
    if (r.L > 0) {
      check(hipMemcpyAsync(r.ls, r.starts, 8 * (size_t)r.L, hipMemcpyHostToDevice, r.st), "starts H2D");
      check(hipMemcpyAsync(r.ll, r.lens, 4 * (size_t)r.L, hipMemcpyHostToDevice, r.st), "lens H2D");
    }
    check(hipMemcpyAsync(r.dlo, up_host_, u.seg_bytes, hipMemcpyHostToDevice, r.st), "segments H2D");
    check(hipMemsetAsync(r.cnt, 0, 8 * sizeof(int64_t), r.st), "counters");
  }
}

// matchers: literal-free scan groups and single-DFA scans (on the side stream: they overlap the
// literal chain and the candidate verification), then the literal prefilter chain.
// fast (request-sized) batches also compute every line's context features there, so the event
// stage needs no feature pass (k_feat_cov over the covered lines sat on the critical path)
bool RequestRunner::run_matchers(Run& r, int attempt) {
  const uint64_t stream = r.stream;
  unsigned long long* c0 = r.c0();
  const bool side = !S_.scans.empty() || S_.n_scan_regs || (r.fast && r.L > 0);
  const bool feat_side = side && r.fast && r.L > 0;
  const uint64_t sst = side ? reinterpret_cast<uint64_t>(side_) : stream;
  if (side) {
    check(hipEventRecord(fork_, r.st), "fork");
    check(hipStreamWaitEvent(side_, fork_, 0), "fork wait");
  }
  for (size_t i = 0; i < S_.scans.size(); ++i)
    scan_multi_dev(r.text, r.nbytes, r.ls, r.ll, r.L, S_.scans[i], r.ver, r.cap_v, c0 + 2, S_.scan_grids[i], sst);
  if (S_.n_scan_regs)
    scan_dev(r.text, r.ls, r.ll, r.L, S_.scan_regs, S_.n_scan_regs, S_.dfa, r.ver, r.cap_v, c0 + 2, sst);
  if (feat_side) feat_all_dev(r.L, r.text, r.ls, r.ll, S_.dfa, S_.ctx_trans, S_.ctx_acc, r.feat, sst);
  if (side) check(hipEventRecord(join_, side_), "join");
  blk_index_dev(r.ls, r.L, r.nblk, r.blk, stream);
  prefilter_dev(r.text, r.nbytes, S_.pf, r.ls, r.L, r.gh, r.cap_g, c0, S_.pf_grid, stream);
  pf_verify_dev(r.gh, r.cap_g, r.text, r.nbytes, S_.pf, r.ls, r.L, r.blk, r.cand, r.cap_c, c0 + 1, stream, c0,
                (int)std::max<int64_t>(16, std::min<int64_t>(8192, r.nbytes >> 13)));
  // the prefilter candidates' verification does not read the scans' buffer: it runs before the join
  bool verified = false;
  if (side && r.fast && r.n <= request_event_cap())
    verified = cand_verify_all_dev(r.cand, r.cap_c, c0 + 1, r.text, r.ls, r.ll, S_.dfa, stream);
  if (side) check(hipStreamWaitEvent(r.st, join_, 0), "join wait");
  r.feat_ready = feat_side;

  if (S_.host_dev)   // the relaxed automata's keys: candidates only, decided by the host side path
    take_host_dev(r.cand, c0 + 1, r.cap_c, r.ver, c0 + 2, r.cap_v, r.text, r.ls, r.ll, S_.dfa, HostSideOut{}, stream);
  // the backtracker regexes' host-verified hits (Engine.host_hits), pre-verified: appended AFTER
  // the relaxed keys are dropped (the drop clears every key of a device-fed regex)
  if (r.ninj > 0) {
    if (attempt == 0) {
      grow<true>(inj_host_, inj_cap_, 8 * (size_t)r.ninj);
      std::memcpy(inj_host_, r.inj, 8 * (size_t)r.ninj);
    }
    check(hipMemcpyAsync(r.inj_dev, inj_host_, 8 * (size_t)r.ninj, hipMemcpyHostToDevice, r.st), "host hits H2D");
    append_keys_dev(r.ver, r.cap_v, c0 + 2, r.inj_dev, r.ninj, stream);
  }
  return verified;
}

// the request's whole tail (hits, events, score, record, publish) as ONE single-workgroup kernel:
// the device-count fast path with its own window, the candidates verified and every line's
// features computed before the join
void RequestRunner::run_tail(Run& r, const HitsArgs& HA) {
  enter_window(r);
  const int64_t E = r.ecap;
  const Results v = r.results(E);
  r.zero_event_inputs(S_, E);
  const EventsArgs EA = r.events_args(S_, E, r.n, r.cnt + 3);
  const ScoreTables T = r.score_tables(S_);
  const FreqIn F{r.ev_rank, r.ev_fkey, r.ring.tot};
  ensure_results(results_bytes(E, r.K1));
  RequestTailOut P;
  P.score = v.score; P.out = r.out; P.E = E; P.K1 = r.K1; P.cnt = r.cnt;
  P.cnt_host = cnt_host_dev_; P.res_host = res_host_dev_;
  P.counts = v.counts; P.K = S_.nkeys; P.now = r.now; P.ring = r.ring;
  P.gate = r.gate();
  request_tail_dev(HA, EA, T, S_.sp, F, P, post_ws_, post_cap_, r.stream);
  recorded_ = true;            // (gated on the device: an overflowing attempt records nothing)
}

void RequestRunner::run_hits(Run& r, const HitsArgs& HA) {
  const size_t need = hits_dev(HA, post_ws_, post_cap_, r.stream);
  if (need > post_cap_) {       // post_ws_ is not used by anything in flight yet
    if (r.fast) throw std::runtime_error("request runner: hit workspace on the small path");
    check(hipStreamSynchronize(r.st), "sync before growth");
    grow<false>(post_ws_, post_cap_, need);
    hits_dev(HA, post_ws_, post_cap_, r.stream);
  }
}

void RequestRunner::run_events(Run& r, int64_t E, int64_t nh_cap, const int64_t* dcnt) {
  r.zero_event_inputs(S_, E);
  const EventsArgs A = r.events_args(S_, E, nh_cap, dcnt);
  const size_t need = events_dev(A, post_ws_, post_cap_, r.stream);
  if (need > post_cap_) {
    if (dcnt) throw std::runtime_error("request runner: event workspace not pre-sized");
    grow<false>(post_ws_, post_cap_, need);   // the stream is idle since the counter read
    events_dev(A, post_ws_, post_cap_, r.stream);
  }
}

// the fused fp64 score over the event stage's outputs; `tot` = the window's carry
void RequestRunner::run_score(Run& r, int64_t E, const int64_t* dcnt, const int64_t* tot) {
  if (E <= 0) return;
  const Results v = r.results(E);
  const FreqIn F{r.ev_rank, r.ev_fkey, tot};
  score_dev(v.line, v.pat, v.seg, F, E, r.score_tables(S_), S_.sp, v.score, nullptr, r.stream,
            dcnt ? dcnt + 1 : nullptr);
}

// shared window: wait for the earlier batches' records, then evict (this batch's carry)
void RequestRunner::enter_window(Run& r) {
  if (r.in_window) return;
  r.turn->wait(r.seq);
  freq_evict(r.ring, r.evict_before, r.stream, true);
  r.in_window = true;
}

// host window (several serving processes): the arrival ticket is drawn once everything that does
// not read the window has FINISHED on the GPU; the section = host eviction + carry copy, the score
// kernel on the pinned carry, the results to the host, the host record. Left on every exit.
void RequestRunner::hw_enter(Run& r) {
  check(hipStreamSynchronize(r.st), "matching before the window section");
  r.hw_seq = r.hw->enter();
  r.hw_now = r.hw->evict_carry(r.now, carry_host_, r.K1);
}

void RequestRunner::hw_leave(Run& r) {
  if (r.hw_seq >= 0) {
    const int64_t q = r.hw_seq;
    r.hw_seq = -1;
    r.hw->leave(q);
  }
}

void RequestRunner::hw_record(Run& r, int64_t ne) {
  if (S_.nkeys > 0)
    r.hw->record_batch(reinterpret_cast<const int64_t*>(res_host_ + 8 * (size_t)ne), S_.nkeys, r.hw_now);
}

// MatchArena.learn: overflow -> the exact rates; otherwise decay toward what batches need
void RequestRunner::learn(const RequestCounts& c, const Run& r, bool ok) {
  auto one = [&](double& rate, int64_t v) {
    const double x = (double)v / (double)std::max<int64_t>(r.L, 1);
    rate = std::max(std::max(x, ok ? rate * 0.5 : rate), 1e-4);
  };
  one(rate_gram_, c.gram);
  one(rate_cand_, c.cand);
  one(rate_ver_, c.ver);
}

// host-count mode: event buffers sized by the counts just read, behind the last attempt's carve
void RequestRunner::finish_host_counts(Run& r, int64_t nh, int64_t ne) {
  const size_t res = results_bytes(ne, r.K1);
  const size_t ws2 = up256(res) + 2 * up256(8 * (size_t)std::max<int64_t>(ne, 1)) +
                     up256((size_t)std::max<int64_t>(r.L, 1)) + up256((size_t)std::max(S_.nseq, 1));
  const size_t base = ws_used_;
  if (base + ws2 > ws_cap_) {
    // the workspace must grow while the inputs / CSR it holds are still needed: move them. The
    // stream is idle (counter read), so copy the used prefix into the new allocation and carve again.
    uint8_t* old = ws_;
    uint8_t* nw = nullptr;
    const size_t ncap = std::max((base + ws2) * 5 / 4, size_t(1) << 20);
    check(hipMalloc(reinterpret_cast<void**>(&nw), ncap), "alloc");
    check(hipMemcpyAsync(nw, old, base, hipMemcpyDeviceToDevice, r.st), "workspace move");
    check(hipStreamSynchronize(r.st), "workspace move");
    check(hipFree(old), "free");
    ws_ = nw;
    ws_cap_ = ncap;
    carve(r);
  }
  ws_used_ = base;
  carve_events(r, ne);
  if (r.hw) {
    run_events(r, ne, nh, nullptr);
    hw_enter(r);
    run_score(r, ne, nullptr, carry_dev_);
  } else {
    enter_window(r);
    run_events(r, ne, nh, nullptr);
    run_score(r, ne, nullptr, r.ring.tot);
    // this batch's per-key counts enter the window (after its own scoring: penalty before record)
    if (S_.nkeys > 0) freq_record(r.results(ne).counts, S_.nkeys, r.now, r.ring, r.stream, true);
    recorded_ = true;
  }
  ensure_results(res);
  check(hipMemcpyAsync(res_host_, r.out, res, hipMemcpyDeviceToHost, r.st), "results D2H");
  check(hipStreamSynchronize(r.st), "results");
  if (r.hw) {
    hw_record(r, ne);
    hw_leave(r);
    recorded_ = true;
  }
  res_bytes_ = res;
}

int64_t RequestRunner::run(uint8_t* host_text, int64_t nbytes, const int64_t* starts, const int32_t* lens, int64_t L,
                           const int32_t* seg_lo, const int32_t* seg_hi, const int64_t* seg_g0, const int64_t* seg_n,
                           int D, const FreqRing& ring, double evict_before, double now, uint64_t stream,
                           int64_t host_cap, Turn* turn, int64_t seq, const int64_t* inj, int64_t ninj,
                           HostWindow* hw, int64_t pre_token) {
  if (hw && turn) throw std::invalid_argument("request runner: a host window or a turn, not both");
  // a shared window: released on every exit, also when a HIP call throws
  struct Release {
    Turn* t;
    int64_t s;
    ~Release() { if (t) t->done(s); }
  } release{turn, seq};
  recorded_ = false;
  check(hipSetDevice(S_.device), "set device");
  Run r{host_text, nbytes, starts, lens, L, D, ring, evict_before, now, stream, turn, seq, inj, ninj, hw,
        reinterpret_cast<hipStream_t>(stream)};
  r.up = upload_layout(nbytes, L, D, S_.nseq);
  r.nblk = (std::max<int64_t>(nbytes, 1) >> kBlkShift) + 2;
  r.lbits = bits_for(std::max<int64_t>(L, 1));
  r.rbits = bits_for(std::max(S_.R, 1));
  r.K1 = std::max(S_.nkeys, 1);
  r.ecap = request_event_cap();
  r.hw_now = now;
  r.ev = S_.ev;
  // the section of a host window is left on every exit
  struct Leave {
    HostWindow* w;
    int64_t* s;
    ~Leave() {             // (a destructor must not throw: a failing turn advance is reported)
      if (!w || *s < 0) return;
      try {
        w->leave(*s);
      } catch (const std::exception& e) {
        std::fprintf(stderr, "[lp] leaving the shared window section failed: %s\n", e.what());
      }
    }
  } leave_guard{hw, &r.hw_seq};

  stage_inputs(r, seg_lo, seg_hi, seg_g0, seg_n, host_cap, pre_token);
  // window eviction first (FrequencyState.carry): the totals it leaves are this batch's carry. Its
  // own launch: as block 0 of the k_fetch launch it showed an unexplained engine p99 of 1.97 ms.
  // A shared window evicts in enter_window(), a host window on the host (hw_enter).
  if (turn == nullptr && hw == nullptr) freq_evict(ring, evict_before, stream, true);
  r.in_window = turn == nullptr;
  if (hw && !carry_host_) {
    check(hipHostMalloc(reinterpret_cast<void**>(&carry_host_), 8 * (size_t)r.K1, kCoherentHost), "pinned carry");
    carry_dev_ = device_view(carry_host_);
  }

  RequestCounts c;
  c.lines = L;
  for (int attempt = 0;; ++attempt) {
    size_attempt(r, attempt);
    carve(r);                                // measure ...
    if (ws_used_ > ws_cap_) {                // ... and carve from a workspace large enough
      check(hipStreamSynchronize(r.st), "sync before growth");   // nothing in flight uses it here
      grow<false>(ws_, ws_cap_, ws_used_);
      carve(r);
    }
    if (r.fast && post_cap_ < 4 * (size_t)std::max<int64_t>(L, 1) + 4096) {   // events' coverage array
      check(hipStreamSynchronize(r.st), "sync before growth");
      grow<false>(post_ws_, post_cap_, 4 * (size_t)std::max<int64_t>(L, 1) + 4096);
    }
    upload(r, attempt);
    const bool verified = run_matchers(r, attempt);
    const HitsArgs HA = r.hits_args(S_, verified);
    const bool tail = r.fast && !hw && verified && r.feat_ready && L > 0;
    if (tail) {
      run_tail(r, HA);
    } else {
      run_hits(r, HA);
      if (r.fast) {          // events + score on the device counters, results published by a kernel
        const int64_t E = r.ecap;
        if (!hw) enter_window(r);
        run_events(r, E, r.n, r.cnt + 3);
        if (hw) hw_enter(r);
        run_score(r, E, r.cnt + 3, hw ? carry_dev_ : ring.tot);
        if (!hw) recorded_ = true;   // (gated on the device: an overflowing attempt records nothing)
        ensure_results(results_bytes(E, r.K1));
        if (hw) {            // recorded on the host
          publish_dev(r.cnt, r.out, E, r.K1, cnt_host_dev_, res_host_dev_, stream);
        } else {             // frequency record + counters + compacted results in host memory: one kernel
          publish_record_dev(r.cnt, r.out, E, r.K1, cnt_host_dev_, res_host_dev_, r.results(E).counts,
                             S_.nkeys, now, ring, r.gate(), stream);
        }
      } else {
        check(hipMemcpyAsync(cnt_host_, r.cnt, 5 * sizeof(int64_t), hipMemcpyDeviceToHost, r.st), "counters D2H");
      }
    }
    check(hipStreamSynchronize(r.st), "counters");   // fast: the only host read; else the mid-batch one
    c.gram = cnt_host_[0]; c.cand = cnt_host_[1]; c.ver = cnt_host_[2];
    c.hits = cnt_host_[3]; c.events = cnt_host_[4];
    const bool ok = c.gram <= r.cap_g && c.cand <= r.cap_c && c.ver <= r.cap_v;
    learn(c, r, ok);
    if (r.fast) recorded_ = false;             // the gate held: nothing was recorded on this attempt
    if (ok && r.fast && c.events <= r.ecap) {  // recorded through the gate; results already read
      if (hw) {                                // the host record of the section (compacted results)
        hw_record(r, c.events);
        hw_leave(r);
      }
      recorded_ = true;
      res_bytes_ = results_bytes(c.events, r.K1);
      break;
    }
    hw_leave(r);                               // an overflowing attempt records nothing: next ticket
    if (ok && !r.fast) {
      finish_host_counts(r, c.hits, c.events);
      break;
    }
    if (attempt > 8) throw std::runtime_error("request runner: matcher capacities did not converge");
  }
  stride_ = c.events;
  counts_ = c;
  return c.events;
}

}  // namespace lp
