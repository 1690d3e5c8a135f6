// aligner.cpp — see aligner.h.
#include "aligner.h"

#include <fcntl.h>
#include <getopt.h>
#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <charconv>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>

#include "band_align.h"
#include "frame_align.h"
#include "common.h"
#include "db_set.h"
#include "query_set.h"
#include "query_tiles.h"
#include "pair_join.h"
#include "read_lca.h"
#include "taxon_profile.h"
#include "worker_pool.h"

namespace ghostm {

// ------------------------------------------------------------------ trace
namespace {
struct TraceEvent {
  double t;
  const char *label;
  uint64_t value;
  std::thread::id thread;
};
std::mutex g_trace_mu;
std::vector<TraceEvent> g_trace;
}  // namespace

double ThreadCpuSeconds() {
  timespec ts;
  clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

bool TraceOn() {
  static const bool on = [] {
    const char *e = getenv("GHOSTM_TRACE");
    return e && *e && strcmp(e, "0") != 0;
  }();
  return on;
}

void TraceMark(const char *label, uint64_t value) {
  if (!TraceOn()) return;
  const double t = NowSeconds();
  std::lock_guard<std::mutex> lk(g_trace_mu);
  g_trace.push_back(TraceEvent{t, label, value, std::this_thread::get_id()});
}

void TraceDump() {
  if (!TraceOn()) return;
  std::lock_guard<std::mutex> lk(g_trace_mu);
  if (g_trace.empty()) return;
  const double t0 = g_trace.front().t;
  const std::thread::id main = g_trace.front().thread;
  for (const TraceEvent &e : g_trace)
    fprintf(stderr, "trace %9.3f %s %-18s %llu\n", (e.t - t0) * 1e3, e.thread == main ? "M" : "F", e.label,
            (unsigned long long)e.value);
  g_trace.clear();
}

unsigned HostThreads() {
  if (const char *e = getenv("GHOSTM_THREADS")) {
    const int v = atoi(e);
    if (v > 0) return (unsigned)v;
  }
  // the CPUs this process may run on: its affinity mask, capped by a cgroup v2
  // CPU quota ("<quota> <period>" in cpu.max; "max" = none)
  unsigned cpus = std::thread::hardware_concurrency();
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) == 0) cpus = (unsigned)CPU_COUNT(&set);
  {
    std::ifstream f("/sys/fs/cgroup/cpu.max");
    std::string quota;
    uint64_t period = 0;
    if (f >> quota >> period && quota != "max" && period > 0) {
      const uint64_t q = strtoull(quota.c_str(), nullptr, 10);
      if (q > 0) cpus = std::min<unsigned>(cpus, (unsigned)std::max<uint64_t>(1, (q + period - 1) / period));
    }
  }
  // shared among the ranks of this node (torchrun sets LOCAL_WORLD_SIZE)
  unsigned ranks = 1;
  if (const char *e = getenv("LOCAL_WORLD_SIZE")) ranks = (unsigned)std::max(1, atoi(e));
  const unsigned share = std::max(1u, cpus) / ranks;
  return std::max(1u, std::min(share, 16u));
}


void ParallelFor(size_t n, unsigned threads,
                 const std::function<void(size_t, size_t, unsigned)> &fn) {
  if (n == 0) return;
  threads = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, n));
  if (threads == 1) {
    fn(0, n, 0);
    return;
  }
  const size_t per = (n + threads - 1) / threads;
  const unsigned pieces = (unsigned)((n + per - 1) / per);
  WorkerPool::Get().Run(pieces, [&](unsigned t) { fn(t * per, std::min(n, (size_t)t * per + per), t); });
}

size_t PieceCount(size_t n, size_t pieces) {
  if (n == 0) return 0;
  const size_t per = (n + std::max<size_t>(1, std::min(pieces, n)) - 1) / std::max<size_t>(1, std::min(pieces, n));
  return (n + per - 1) / per;
}

void ParallelForPieces(size_t n, size_t pieces, unsigned threads,
                       const std::function<void(size_t, size_t, unsigned)> &fn) {
  const size_t np = PieceCount(n, pieces);
  if (np == 0) return;
  const size_t per = (n + np - 1) / np;
  if (threads <= 1 || np == 1) {
    for (size_t t = 0; t < np; ++t) fn(t * per, std::min(n, t * per + per), (unsigned)t);
    return;
  }
  WorkerPool::Get().Run((unsigned)np, [&](unsigned t) { fn(t * per, std::min(n, (size_t)t * per + per), t); },
                        threads);
}

// ------------------------------------------------------------------ TaskQueue
TaskQueue::TaskQueue() : worker_([this] { Loop(); }) {}

TaskQueue::~TaskQueue() {
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  worker_.join();
}

void TaskQueue::Submit(std::function<void()> fn) {
  {
    std::lock_guard<std::mutex> lk(mu_);
    tasks_.push_back(std::move(fn));
  }
  cv_.notify_one();
}

void TaskQueue::Drain() {
  std::unique_lock<std::mutex> lk(mu_);
  idle_.wait(lk, [this] { return tasks_.empty() && !busy_; });
  if (error_) {
    std::exception_ptr e = error_;
    error_ = nullptr;
    std::rethrow_exception(e);
  }
}

void TaskQueue::Loop() {
  for (;;) {
    std::function<void()> fn;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [this] { return stop_ || !tasks_.empty(); });
      if (tasks_.empty()) return;
      fn = std::move(tasks_.front());
      tasks_.pop_front();
      busy_ = true;
    }
    try {
      fn();
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu_);
      if (!error_) error_ = std::current_exception();
    }
    {
      std::lock_guard<std::mutex> lk(mu_);
      busy_ = false;
    }
    idle_.notify_all();
  }
}

// ------------------------------------------------------------------ options
AlignerOptions ParseAlignerOptions(int argc, char **argv) {
  AlignerOptions o;
  std::string matrix_file = "BLOSUM62";
  optind = 1;
  opterr = 1;
  int c;
  while ((c = getopt(argc, argv, "b:d:D:e:E:G:i:l:M:o:r:s:t:S:L:y:v")) >= 0) {
    switch (c) {
      case 'b': o.best = atoi(optarg); break;
      case 'd': o.db_prefix = optarg; break;
      case 'D': o.device = atoi(optarg); break;
      case 'e': o.extend = atoi(optarg); break;
      case 'E': o.extend_gap = -atoi(optarg); break;
      case 'G': o.open_gap = -atoi(optarg); break;
      case 'i': o.query_prefix = optarg; break;
      case 'S': o.start_query_chunk = atoi(optarg); break;
      case 'L': o.end_query_chunk = atoi(optarg); break;
      case 'l': o.max_list_length = atoi(optarg) * (1 << 20); break;
      case 'M': matrix_file = optarg; break;
      case 'o': o.output_file = optarg; break;
      case 'r': {
        const int lr = (int)log2(atoi(optarg));
        o.log_region = lr < 1 ? 1 : lr;
        break;
      }
      case 's': o.shift = atoi(optarg); break;
      case 't': o.threshold = atoi(optarg); break;
      case 'y': o.output_style = atoi(optarg); break;
      case 'v': o.verbose = true; break;
      default: throw std::invalid_argument("");
    }
  }
  // test hook: -l in candidates instead of MiB units (exercises batch cuts on
  // small inputs); the oracle honours the same variable
  if (const char *e = getenv("GHOSTM_MAX_LIST_OVERRIDE")) o.max_list_length = (uint32_t)strtoul(e, nullptr, 10);
  o.matrix = ReadScoreMatrix(matrix_file);
  // 6 to 9, 12 to 15, 20 and 21: style 0's E-value and bit score; 10, 11 and 16 to 19 (the pile-ups) print none, like 1 and 2
  if (o.output_style == 0 || (o.output_style >= 6 && o.output_style <= 9) ||
      (o.output_style >= 12 && o.output_style <= 15) || o.output_style == 20 || o.output_style == 21) {
    // extension: GHOSTM_KARLIN=ungapped prices combinations the
    // reference's table lacks with the matrix's ungapped ideal parameters
    // (karlin_params.cpp); unset, they throw as the reference does
    const char *kp = getenv("GHOSTM_KARLIN");
    if (kp && std::string(kp) == "ungapped") {
      try {
        o.karlin = GappedKarlinParams(o.matrix, o.open_gap, o.extend_gap);
      } catch (std::invalid_argument &) {
        o.karlin = UngappedKarlinParams(o.matrix);
      }
    } else {
      o.karlin = GappedKarlinParams(o.matrix, o.open_gap, o.extend_gap);
    }
  }
  return o;
}

// ------------------------------------------------------------------ shards
void ShardCuts(uint64_t n, const uint32_t *weight, const uint8_t *group_start, uint32_t world, uint64_t *cuts) {
  if (world == 0) throw std::invalid_argument("world must be >= 1");
  std::vector<uint64_t> prefix(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) prefix[i + 1] = prefix[i] + weight[i];
  const unsigned __int128 total = prefix[n];
  cuts[0] = 0;
  for (uint32_t r = 1; r < world; ++r) {
    // first group start at or after the previous cut whose prefix weight
    // reaches total * r / world (exact integer comparison)
    uint64_t c = cuts[r - 1];
    while (c < n && !((c == 0 || group_start[c]) && (unsigned __int128)prefix[c] * world >= total * r)) ++c;
    cuts[r] = c;
  }
  cuts[world] = n;
}

// The CPU path's batch cuts (aligner.cpp:383-521 driven by Execute's loop at
// 131-171): a query whose candidates push the running total above -l is carried
// into the next batch; the loop stops at the first empty batch, so a carried last
// query is dropped, exactly as the reference does.
std::vector<Batch> CpuBatches(const std::vector<uint32_t> &counts, uint64_t max_list) {
  std::vector<Batch> out;
  const uint32_t n = (uint32_t)counts.size();
  uint32_t next = 0;
  int64_t carry = -1;
  for (;;) {
    if (next == n) break;
    uint32_t first = next;
    uint64_t total = 0;
    if (carry >= 0) {
      first = (uint32_t)carry;
      total = counts[carry];
    }
    carry = -1;
    uint32_t i = next;
    bool cut = false;
    for (; i < n; ++i) {
      total += counts[i];
      if (total > max_list) { cut = true; break; }
    }
    const uint64_t cands = cut ? total - counts[i] : total;
    const uint32_t stop = cut ? i : n;
    if (cut) { next = i + 1; carry = i; } else { next = n; }
    if (cands == 0) break;
    out.push_back(Batch{first, stop});
  }
  return out;
}

namespace {
// FNV-1a over a slice's candidate counts: a shard's runs must see the counts
// its batch plan was made from
uint64_t CountsHash(const uint32_t *c, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) {
    h ^= c[i];
    h *= 1099511628211ull;
  }
  return h;
}
}  // namespace

// Name groups (consecutive equal names, merged into one result list:
// aligner.cpp:697-700) and (qlen) WriteOutput's query lengths of one query chunk.
void Session::PrepareQueryChunk(QueryData *qd, bool qlen) {
  QueryData &q = *qd;
  const uint32_t n = q.chunk.nseq, L = q.chunk.L;
  q.group_end.assign(n, 0);
  q.group_first.clear();
  q.group_last.clear();
  for (uint32_t i = n; i-- > 0;) {
    q.group_end[i] = (i + 1 < n && q.chunk.names[i + 1] == q.chunk.names[i]) ? q.group_end[i + 1] : i + 1;
  }
  for (uint32_t i = 0; i < n; i = q.group_end[i]) {
    q.group_first.push_back(i);
    q.group_last.push_back(q.group_end[i] - 1);
  }
  if (!qlen) return;
  q.qlen.assign(n, 1);
  for (uint32_t i = 0; i < n; ++i) q.qlen[i] = QueryResidues(&q.chunk.seq[(size_t)i * L], L);
}

// WriteOutput's query lengths of every loaded chunk on the worker pool, in
// blocks of rows (a row's last byte per 127: ~9 ms per 500 K-query chunk on one
// thread, the largest part of reading a chunk once its names are a NameTable).
void Session::QueryLengths(std::vector<QueryData *> chunks) {
  constexpr uint32_t kRows = 1u << 12;
  std::vector<std::pair<QueryData *, uint32_t>> blocks;
  for (QueryData *q : chunks) {
    q->qlen.assign(q->chunk.nseq, 1);
    for (uint32_t r = 0; r < q->chunk.nseq; r += kRows) blocks.emplace_back(q, r);
  }
  ParallelFor(blocks.size(), std::max(1u, threads_), [&](size_t b, size_t e, unsigned) {
    for (size_t k = b; k < e; ++k) {
      QueryData &q = *blocks[k].first;
      const uint32_t L = q.chunk.L, r1 = std::min(q.chunk.nseq, blocks[k].second + kRows);
      for (uint32_t i = blocks[k].second; i < r1; ++i) q.qlen[i] = QueryResidues(&q.chunk.seq[(size_t)i * L], L);
    }
  });
}

// The batch plan of a slice against DB chunk di, from the counts of its WHOLE
// chunk: the unsharded run's batches (aligner.cpp:131-171, 511-514), which every
// shard replays on its own queries (see Passes).
void Session::PlanFromCounts(QueryData &q, size_t di, const std::vector<uint32_t> &chunk_counts, uint32_t n) {
  if (q.plan.size() <= di) {
    q.plan.resize(di + 1);
    q.plan_sum.resize(di + 1);
    q.plan_hash.resize(di + 1);
  }
  q.plan[di] = CpuBatches(chunk_counts, opt_.max_list_length);
  uint64_t sum = 0;
  for (uint32_t i = 0; i < n; ++i) sum += chunk_counts[q.slice_lo + i];
  q.plan_sum[di] = sum;
  q.plan_hash[di] = CountsHash(chunk_counts.data() + q.slice_lo, n);
  q.planned = true;
}

// Without a collective: the shard counts every query of each chunk it touches
// itself (K1 on the whole chunk, once), then keeps only its own range. The
// chunks' queries are cut into `world` contiguous ranges of about equal
// residues, at name-group starts (groups never span chunks: the reference
// merges per chunk, aligner.cpp:697-700).
void Session::ApplyShard(uint32_t rank, uint32_t world) {
  DeviceModule &dev = DeviceModule::Get();
  std::vector<uint32_t> weight;
  std::vector<uint8_t> start;
  for (const QueryData &q : queries_) {
    const QueryChunk &c = q.chunk;
    for (uint32_t i = 0; i < c.nseq; ++i) {
      weight.push_back(q.qlen[i]);
      start.push_back(i == 0 || c.names[i] != c.names[i - 1]);
    }
  }
  std::vector<uint64_t> cuts(world + 1);
  ShardCuts(weight.size(), weight.data(), start.data(), world, cuts.data());
  const uint64_t lo = cuts[rank], hi = cuts[rank + 1];
  shard_begin_ = lo;
  shard_end_ = hi;
  SeedConfig sc;
  sc.threshold = opt_.threshold;
  sc.shift = opt_.shift;
  sc.log_region = opt_.log_region;
  std::vector<QueryData> kept;
  uint64_t at = 0;  // index of the chunk's first query over the loaded chunks
  for (QueryData &q : queries_) {
    QueryChunk &c = q.chunk;
    const uint64_t chunk_end = at + c.nseq;
    const uint64_t b = std::max<uint64_t>(lo, at), e = std::min<uint64_t>(hi, chunk_end);
    if (b < e) {
      const uint32_t i0 = (uint32_t)(b - at), n = (uint32_t)(e - b);
      // the whole chunk's counts against every DB chunk -> its batch plan
      q.slice_lo = i0;
      q.chunk_nseq = c.nseq;
      {
        // the whole chunk on the device while it is counted; freed on every exit
        std::unique_ptr<DevQuery, std::function<void(DevQuery *)>> full(
            dev.UploadQuery(c.seq.data(), c.nseq, c.L), [&dev](DevQuery *p) { dev.Free(p); });
        std::vector<uint32_t> counts;
        std::vector<uint64_t> offsets;
        for (size_t di = 0; di < dbs_.size(); ++di) {
          sc.seed_mask = dbs_[di].chunk.seed;
          dev.Seed(full.get(), dbs_[di].dev, sc, &counts, &offsets);
          PlanFromCounts(q, di, counts, n);
        }
      }
      c.seq.Own(std::vector<uint8_t>(c.seq.begin() + (size_t)i0 * c.L, c.seq.begin() + (size_t)(i0 + n) * c.L));
      c.names = c.names.Slice(i0, n);
      c.nseq = n;
      q.global_base += i0;
      PrepareQueryChunk(&q);
      kept.push_back(std::move(q));
    }
    at = chunk_end;
  }
  queries_.swap(kept);
}

// With a collective: every rank has counted its own slices; the ranks
// all-gather their candidate totals per (query chunk, DB chunk). A chunk whose
// total fits -l is one batch, as in the unsharded run; otherwise the ranks
// all-gather the chunk's per-query counts and cut it with the CPU rule.
// chunk_nseq[c] = queries of chunk c, rank_lo[c][r] = rank r's first query in
// chunk c (rank_lo[c][world] = chunk_nseq[c]).
void Session::PlanExchange(uint32_t rank, uint32_t world, const ShardExchange &ex,
                           const std::vector<uint32_t> &chunk_nseq,
                           const std::vector<std::vector<uint64_t>> &rank_lo) {
  DeviceModule &dev = DeviceModule::Get();
  const size_t nc = chunk_nseq.size(), nd = dbs_.size();
  SeedConfig sc;
  sc.threshold = opt_.threshold;
  sc.shift = opt_.shift;
  sc.log_region = opt_.log_region;
  // this rank's counts per (chunk, DB chunk); queries_ holds its slices in chunk order
  std::vector<QueryData *> slice(nc, nullptr);
  {
    size_t k = 0;
    for (size_t c = 0; c < nc; ++c)
      if (rank_lo[c][rank] < rank_lo[c][rank + 1]) slice[c] = &queries_.at(k++);
    if (k != queries_.size()) throw Error("shard slices out of order");
  }
  std::vector<std::vector<uint32_t>> mine(nc * nd);
  // the candidate totals per (chunk, DB chunk), then this rank's ok flag: a
  // rank whose counting fails still takes part in the gather, and every rank
  // then fails
  const size_t np = nc * nd;
  std::vector<uint64_t> sums(np + 1, 0);
  std::string err;
  try {
    for (size_t c = 0; c < nc; ++c) {
      if (!slice[c]) continue;
      std::vector<uint64_t> offsets;
      for (size_t di = 0; di < nd; ++di) {
        sc.seed_mask = dbs_[di].chunk.seed;
        sums[c * nd + di] = dev.Seed(slice[c]->dev, dbs_[di].dev, sc, &mine[c * nd + di], &offsets);
      }
    }
  } catch (std::exception &e) {
    err = e.what();
    if (err.empty()) err = "shard session: counting failed";
  }
  sums[np] = err.empty() ? 1 : 0;
  auto gather = [&](const void *send, uint64_t bytes, void *recv, const std::vector<uint64_t> &sizes) {
    if (ex.fn(ex.ctx, send, bytes, recv, sizes.data()) != 0) throw Error("shard exchange (all-gather) failed");
  };
  std::vector<uint64_t> all(world * (np + 1));
  gather(sums.data(), sums.size() * 8, all.data(), std::vector<uint64_t>(world, sums.size() * 8));
  if (!err.empty()) throw Error(err);
  for (uint32_t r = 0; r < world; ++r)
    if (all[r * (np + 1) + np] != 1)
      throw Error("shard session: rank " + std::to_string(r) + " failed counting its queries");
  std::vector<uint64_t> total(np, 0);
  for (uint32_t r = 0; r < world; ++r)
    for (size_t p = 0; p < np; ++p) total[p] += all[r * (np + 1) + p];
  // pairs that need the whole chunk's counts: more than one batch
  std::vector<size_t> wide;
  for (size_t p = 0; p < nc * nd; ++p)
    if (total[p] > opt_.max_list_length) wide.push_back(p);
  std::vector<std::vector<uint32_t>> chunk_counts(nc * nd);
  if (!wide.empty()) {
    std::vector<uint64_t> sizes(world, 0);
    for (uint32_t r = 0; r < world; ++r)
      for (size_t p : wide) sizes[r] += (rank_lo[p / nd][r + 1] - rank_lo[p / nd][r]) * 4;
    std::vector<uint32_t> send;
    for (size_t p : wide) send.insert(send.end(), mine[p].begin(), mine[p].end());
    if (send.size() * 4 != sizes[rank]) throw Error("shard exchange: slice sizes disagree");
    uint64_t recv_total = 0;
    for (uint64_t s : sizes) recv_total += s;
    std::vector<uint32_t> recv(recv_total / 4);
    gather(send.data(), send.size() * 4, recv.data(), sizes);
    // rank r's block holds its part of every wide pair in order
    uint64_t block = 0;
    for (uint32_t r = 0; r < world; ++r) {
      uint64_t at = block;
      for (size_t p : wide) {
        const uint64_t n = rank_lo[p / nd][r + 1] - rank_lo[p / nd][r];
        chunk_counts[p].insert(chunk_counts[p].end(), recv.begin() + at, recv.begin() + at + n);
        at += n;
      }
      block += sizes[r] / 4;
    }
  }
  for (size_t c = 0; c < nc; ++c) {
    QueryData *q = slice[c];
    if (!q) continue;
    for (size_t di = 0; di < nd; ++di) {
      const size_t p = c * nd + di;
      if (q->plan.size() <= di) {
        q->plan.resize(di + 1);
        q->plan_sum.resize(di + 1);
        q->plan_hash.resize(di + 1);
      }
      if (total[p] > opt_.max_list_length) {
        if (chunk_counts[p].size() != chunk_nseq[c]) throw Error("shard exchange: chunk counts incomplete");
        q->plan[di] = CpuBatches(chunk_counts[p], opt_.max_list_length);
      } else if (total[p] > 0) {
        q->plan[di] = {Batch{0, chunk_nseq[c]}};  // CpuBatches of a chunk within -l
      } else {
        q->plan[di].clear();
      }
      q->plan_sum[di] = sums[p];
      q->plan_hash[di] = CountsHash(mine[p].data(), mine[p].size());
    }
    q->planned = true;
  }
}

std::vector<Batch> Session::Passes(QueryData &q, size_t di, const std::vector<uint32_t> &counts,
                                   uint64_t total) const {
  if (!q.planned) {
    // within -l the rule makes one batch (none without candidates): no scan
    if (total <= opt_.max_list_length)
      return total ? std::vector<Batch>{Batch{0, (uint32_t)counts.size()}} : std::vector<Batch>{};
    return CpuBatches(counts, opt_.max_list_length);
  }
  uint64_t sum = 0;
  for (uint32_t c : counts) sum += c;
  if (di >= q.plan.size() || sum != q.plan_sum[di] || CountsHash(counts.data(), counts.size()) != q.plan_hash[di])
    throw Error("shard session: candidate counts differ from its batch plan");
  const uint32_t lo = q.slice_lo, hi = lo + q.chunk.nseq;
  std::vector<Batch> out;
  for (const Batch &b : q.plan[di])
    out.push_back(Batch{std::clamp(b.q0, lo, hi) - lo, std::clamp(b.q1, lo, hi) - lo});
  return out;
}

// ------------------------------------------------------------------ session
Session::Session(const AlignerOptions &opt, uint32_t shard_rank, uint32_t shard_world, const ShardExchange *ex)
    : opt_(opt) {
  threads_ = HostThreads();
  if (shard_world == 0 || shard_rank >= shard_world) throw std::invalid_argument("shard rank outside the world");
  CreateOrFree(shard_rank, shard_world, ex);
}

Session::Session(const AlignerOptions &opt, DbOnly) : opt_(opt), db_only_(true) {
  threads_ = HostThreads();
  if (!opt.query_prefix.empty() || opt.start_query_chunk != UINT32_MAX || opt.end_query_chunk != UINT32_MAX)
    throw std::invalid_argument("a database session takes no -i, -S or -L: its queries come from SetQueries");
  CreateOrFree(0, 1, nullptr);
}

Session::Session(const AlignerOptions &opt, NoDb) : opt_(opt), no_db_(true) {
  threads_ = HostThreads();
  if (!opt.db_prefix.empty())
    throw std::invalid_argument("a session without a database takes no -d: its database comes from SetDb");
  CreateOrFree(0, 1, nullptr);
}

void Session::CreateOrFree(uint32_t shard_rank, uint32_t shard_world, const ShardExchange *ex) {
  try {
    Create(shard_rank, shard_world, ex);
  } catch (...) {
    // a throwing constructor runs no destructor: free the resident chunks here
    DeviceModule &dev = DeviceModule::Get();
    for (QueryData &q : queries_) dev.Free(q.dev);
    for (DbData &d : dbs_) dev.Free(d.dev);
    queries_.clear();
    dbs_.clear();
    throw;
  }
}

void Session::Create(uint32_t shard_rank, uint32_t shard_world, const ShardExchange *ex) {
  shard_world_ = shard_world;
  const bool local = shard_world > 1 && ex && ex->fn;  // rank-local reads + exchange
  std::vector<uint32_t> chunk_nseq;
  std::vector<std::vector<uint64_t>> rank_lo;
  if (!local) {
    Load(shard_rank, shard_world, false, &chunk_nseq, &rank_lo);
  } else {
    // a rank whose loading fails still joins the creation header exchange with
    // its error flag set, so every rank fails together instead of its peers
    // waiting in the plan's all-gather for a rank that never comes
    std::string err;
    try {
      Load(shard_rank, shard_world, true, &chunk_nseq, &rank_lo);
    } catch (std::exception &e) {
      err = e.what();
      if (err.empty()) err = "shard session creation failed";
    }
    AgreeOnCreate(shard_rank, shard_world, *ex, err, chunk_nseq, rank_lo);
    PlanExchange(shard_rank, shard_world, *ex, chunk_nseq, rank_lo);
  }
  TraceMark("create_sync");
  DeviceModule::Get().Synchronize();
  TraceMark("uploaded");
  formatter_.reset(new TaskQueue());
}

// Every rank's view of the job must be the same before the plan's all-gather
// sizes its buffers from it: a fixed-size header per rank (ok flag, query
// chunks, DB chunks, queries, a hash of every chunk's size and of the shard
// cuts) is all-gathered first. Any rank's failure or any disagreement throws on
// every rank.
void Session::AgreeOnCreate(uint32_t rank, uint32_t world, const ShardExchange &ex, const std::string &err,
                            const std::vector<uint32_t> &chunk_nseq,
                            const std::vector<std::vector<uint64_t>> &rank_lo) {
  constexpr size_t kWords = 8;
  uint64_t mine[kWords] = {0};
  mine[0] = err.empty() ? 1 : 0;
  if (err.empty()) {
    mine[1] = chunk_nseq.size();
    mine[2] = dbs_.size();
    for (uint32_t n : chunk_nseq) mine[3] += n;
    mine[4] = CountsHash(chunk_nseq.data(), chunk_nseq.size());
    std::vector<uint32_t> cuts;
    for (const std::vector<uint64_t> &lo : rank_lo)
      for (uint64_t x : lo) cuts.push_back((uint32_t)x);
    mine[5] = CountsHash(cuts.data(), cuts.size());
    mine[6] = db_sum_u32_;
    mine[7] = world;
  }
  std::vector<uint64_t> all(world * kWords);
  const std::vector<uint64_t> sizes(world, sizeof(mine));
  if (ex.fn(ex.ctx, mine, sizeof(mine), all.data(), sizes.data()) != 0)
    throw Error("shard exchange (creation header all-gather) failed");
  if (!err.empty()) throw Error(err);
  for (uint32_t r = 0; r < world; ++r) {
    const uint64_t *h = &all[r * kWords];
    if (h[0] != 1) throw Error("shard session: rank " + std::to_string(r) + " failed at creation");
    for (size_t k = 1; k < kWords; ++k)
      if (h[k] != mine[k])
        throw Error("shard session: rank " + std::to_string(r) + " sees a different query/DB set than rank " +
                    std::to_string(rank));
  }
}

// Reads and uploads the query and DB chunks (a rank-local shard: only its own
// slice of the queries) and, for a rank-local shard, returns the chunks' sizes
// and every rank's first query per chunk.
void Session::Load(uint32_t shard_rank, uint32_t shard_world, bool local, std::vector<uint32_t> *chunk_nseq_out,
                   std::vector<std::vector<uint64_t>> *rank_lo_out) {
  std::vector<uint32_t> &chunk_nseq = *chunk_nseq_out;
  std::vector<std::vector<uint64_t>> &rank_lo = *rank_lo_out;
  DeviceModule &dev = DeviceModule::Get();
  TraceMark("create");
  dev.Bind(opt_.device);
  TraceMark("bound");
  // the staged uploads' host copies on the worker pool, 1 MB per piece
  const unsigned copiers = std::max(1u, std::min(threads_, 8u));
  dev.SetHostCopy([copiers](void *dst, const void *src, size_t n) {
    const size_t piece = 1u << 20, pieces = (n + piece - 1) / piece;
    ParallelFor(pieces, copiers, [&](size_t b, size_t e, unsigned) {
      const size_t lo = b * piece, hi = std::min(n, e * piece);
      std::memcpy(static_cast<char *>(dst) + lo, static_cast<const char *>(src) + lo, hi - lo);
    });
  });
  dev.SetHostParallel([copiers](size_t parts, const std::function<void(size_t)> &fn) {
    ParallelFor(parts, copiers, [&](size_t b, size_t e, unsigned) {
      for (size_t k = b; k < e; ++k) fn(k);
    });
  });
  dev.SetMatrix(opt_.matrix.m.data());

  // query chunks: -S start (or 0) .. -L end, as Execute walks them
  // (aligner.cpp:98-204), and every DB chunk; the chunk files are read on
  // parallel threads, then the chunks up to the first missing one are kept
  QueryFile qf(opt_.query_prefix);
  if (db_only_) qf.division = 0;  // a database session: no query files
  if (no_db_ && opt_.query_prefix.empty()) qf.division = 0;  // ... or neither input yet
  uint32_t id = opt_.start_query_chunk == UINT32_MAX ? 0 : opt_.start_query_chunk;
  uint32_t base = 0;
  for (uint32_t k = 0; k < id && k < qf.division; ++k) {
    std::ifstream f((qf.prefix + "_" + std::to_string(k) + ".inf").c_str(), std::ios::binary);
    uint32_t n = 0;
    if (f) f.read(reinterpret_cast<char *>(&n), 4);
    base += n;
  }
  // chunk `id`, then the following ones up to -L (at least `id` itself)
  uint32_t nq_chunks = 0;
  if ((int64_t)id < (int64_t)qf.division) {
    const uint64_t last = std::min<uint64_t>(opt_.end_query_chunk, (uint64_t)qf.division - 1);
    nq_chunks = (uint32_t)(last >= id ? last - id + 1 : 1);
  }
  DbFile df(opt_.db_prefix);
  const uint32_t nd_chunks = (int64_t)df.division > 0 && !no_db_ ? (uint32_t)df.division : 0u;
  std::vector<QueryData> qread(nq_chunks);
  std::vector<QueryChunkIndex> qidx(local ? nq_chunks : 0);
  std::vector<DbData> dread(nd_chunks);
  std::vector<char> qok(nq_chunks, 0), dok(nd_chunks, 0);
  // chunks uploaded here but not (yet) handed to queries_/dbs_ are freed on every
  // exit, the error exits included (a chunk handed over has its handle nulled
  // here; the constructor frees queries_/dbs_ if creation fails later)
  struct Unadopted {
    std::vector<QueryData> &q;
    std::vector<DbData> &d;
    ~Unadopted() {
      DeviceModule &m = DeviceModule::Get();
      for (QueryData &x : q)
        if (x.dev) m.Free(x.dev);
      for (DbData &x : d)
        if (x.dev) m.Free(x.dev);
    }
  } unadopted{qread, dread};
  // (each query chunk's name groups and WriteOutput lengths are derived on its
  // reading thread too; a rank-local shard only indexes the query chunks here).
  // A DB chunk is uploaded by its reading thread as soon as it is read, one
  // upload at a time (the staging buffers are shared), while the query chunks
  // are still being read (cfg3: the 34 MB DB and index upload took 1.5 ms of a
  // 4.1 ms session create after every read, profiles/r5ad/)
  std::mutex upload_mu;
  // host copies resident on the device are dropped on a thread of their own
  // after creation (unmapping ~40 MB of chunk files took ~0.3 ms per 12.7 MB
  // on the critical path, and under the upload lock)
  std::mutex drop_mu;
  std::vector<std::shared_ptr<const void>> drop;
  auto drop_later = [&](std::shared_ptr<const void> h) {
    std::lock_guard<std::mutex> lock(drop_mu);
    drop.push_back(std::move(h));
  };
  struct DropInBackground {
    std::vector<std::shared_ptr<const void>> &d;
    ~DropInBackground() {
      if (d.empty()) return;
      try {
        std::thread([h = std::move(d)]() mutable { h.clear(); }).detach();
      } catch (...) {
        d.clear();  // no thread: drop them here
      }
    }
  } drop_in_background{drop};
  auto upload_db = [&](DbData &d) {
    {
      std::lock_guard<std::mutex> lock(upload_mu);
      const DbChunk &c = d.chunk;
      d.dev = dev.UploadDb(c.seq.data(), c.len, c.keys_count.data(), c.kcl, c.positions.data(), c.npos);
      if (c.nseq) dev.SetDbSubjects(d.dev, c.starts.data(), c.nseq);
    }
    // resident on the device from here; the host keeps names and starts
    drop_later(d.chunk.seq.Detach());
    drop_later(d.chunk.keys_count.Detach());
    drop_later(d.chunk.positions.Detach());
  };
  auto upload_query = [&](QueryData &q) {
    std::lock_guard<std::mutex> lock(upload_mu);
    q.dev = dev.UploadQuery(q.chunk.seq.data(), q.chunk.nseq, q.chunk.L);
    dev.SetQueryGroups(q.dev, q.group_first.data(), q.group_last.data(), (uint32_t)q.group_first.size());
  };
  ParallelFor(nq_chunks + nd_chunks, std::max<unsigned>(1u, std::min(threads_, 8u)),
              [&](size_t b0, size_t e0, unsigned) {
                // DB chunks first (they are listed after the query chunks)
                for (size_t j = b0; j < e0; ++j) {
                  const size_t k = nq_chunks + nd_chunks - 1 - j;
                  if (k < nq_chunks && local) {
                    qok[k] = qf.IndexChunk(id + (uint32_t)k, &qidx[k]);
                  } else if (k < nq_chunks) {
                    qok[k] = qf.ReadChunk(id + (uint32_t)k, &qread[k].chunk);
                    if (qok[k]) PrepareQueryChunk(&qread[k], false);
                    TraceMark("q_chunk_read", k);
                    // an unsharded session uploads the chunk here too (a sharded
                    // one keeps only its slice, below)
                    if (qok[k] && shard_world == 1) {
                      upload_query(qread[k]);
                      TraceMark("q_chunk_up", k);
                    }
                  } else {
                    DbData &d = dread[k - nq_chunks];
                    dok[k - nq_chunks] = df.ReadChunk((uint32_t)(k - nq_chunks), &d.chunk);
                    TraceMark("db_chunk_read", k - nq_chunks);
                    if (dok[k - nq_chunks]) upload_db(d);
                    TraceMark("db_chunk_up", k - nq_chunks);
                  }
                }
              });
  uint32_t nchunks = 0;
  while (nchunks < nq_chunks && qok[nchunks]) ++nchunks;
  if (nchunks == 0 && !db_only_ && !(no_db_ && opt_.query_prefix.empty()))
    throw std::runtime_error("[Aligner] error: don't find query file.");
  if (!local) {
    std::vector<QueryData *> chunks;
    for (uint32_t k = 0; k < nchunks; ++k) chunks.push_back(&qread[k]);
    QueryLengths(chunks);
  }
  TraceMark("queries_read", nchunks);

  db_sum_u32_ = no_db_ ? 0 : (uint32_t)df.sum_length;
  uint32_t dbase = 0;
  uint32_t nd_kept = 0;
  for (; nd_kept < nd_chunks && dok[nd_kept]; ++nd_kept) {
    dread[nd_kept].global_base = dbase;
    dbase += dread[nd_kept].chunk.nseq;
    dbs_.push_back(std::move(dread[nd_kept]));
    dread[nd_kept].dev = nullptr;
  }
  // chunks read past a missing one are not used (freed by `unadopted`)
  if (dbs_.empty() && !no_db_) throw std::runtime_error("[Aligner] error: don't find db file.");
  TraceMark("db_read", dbs_.size());
  {
    std::vector<uint32_t> bases;
    for (const DbData &d : dbs_) bases.push_back(d.global_base);
    // DB chunk ids are the indices into dbs_ (chunks are read from 0 in order)
    for (size_t k = 0; k < dbs_.size(); ++k)
      if (dbs_[k].chunk.id != k) throw Error("DB chunk ids out of order");
    dev.SetChunkBases(bases.data(), (uint32_t)bases.size());
    TraceMark("bases_set");
  }

  if (local) {
    // the cut over every selected query from the chunk indices, then only this
    // rank's rows and names are read
    std::vector<uint32_t> weight;
    std::vector<uint8_t> start;
    for (uint32_t k = 0; k < nchunks; ++k) {
      weight.insert(weight.end(), qidx[k].qlen.begin(), qidx[k].qlen.end());
      start.insert(start.end(), qidx[k].group_start.begin(), qidx[k].group_start.end());
    }
    std::vector<uint64_t> cuts(shard_world + 1);
    ShardCuts(weight.size(), weight.data(), start.data(), shard_world, cuts.data());
    shard_begin_ = cuts[shard_rank];
    shard_end_ = cuts[shard_rank + 1];
    std::vector<uint32_t> read;  // chunks holding queries of this rank
    uint64_t at = 0;
    uint32_t cbase = base;
    chunk_nseq.resize(nchunks);
    rank_lo.resize(nchunks);
    for (uint32_t k = 0; k < nchunks; ++k) {
      const uint32_t n = qidx[k].nseq;
      chunk_nseq[k] = n;
      for (uint32_t r = 0; r <= shard_world; ++r)
        rank_lo[k].push_back(std::min<uint64_t>(n, cuts[r] > at ? cuts[r] - at : 0));
      if (rank_lo[k][shard_rank] < rank_lo[k][shard_rank + 1]) {
        qread[k].slice_lo = (uint32_t)rank_lo[k][shard_rank];
        qread[k].chunk_nseq = n;
        qread[k].global_base = cbase + qread[k].slice_lo;
        read.push_back(k);
      }
      at += n;
      cbase += n;
    }
    ParallelFor(read.size(), std::max<unsigned>(1u, std::min(threads_, 8u)), [&](size_t b, size_t e, unsigned) {
      for (size_t j = b; j < e; ++j) {
        const uint32_t k = read[j];
        qidx[k].ReadSlice(qread[k].slice_lo, (uint32_t)(rank_lo[k][shard_rank + 1] - qread[k].slice_lo),
                          &qread[k].chunk);
        PrepareQueryChunk(&qread[k], false);
      }
    });
    {
      std::vector<QueryData *> chunks;
      for (uint32_t k : read) chunks.push_back(&qread[k]);
      QueryLengths(chunks);
    }
    for (uint32_t k : read) {
      queries_.push_back(std::move(qread[k]));
      qread[k].dev = nullptr;
    }
    TraceMark("slices_read", queries_.size());
  } else {
    for (uint32_t k = 0; k < nchunks; ++k) {
      qread[k].global_base = base;
      base += qread[k].chunk.nseq;
      queries_.push_back(std::move(qread[k]));
      qread[k].dev = nullptr;
    }
    if (shard_world > 1) ApplyShard(shard_rank, shard_world);  // may leave no queries
  }

  for (QueryData &q : queries_) {
    if (!q.dev) upload_query(q);  // (uploaded while reading when unsharded)
    drop_later(q.chunk.seq.Detach());  // resident on the device (qlen and names stay on the host)
  }
  TraceMark("queries_released");
  // query chunks read past a missing one are not used (freed by `unadopted`)
}

namespace {
struct MergeItem {
  uint32_t score;
  uint32_t end;       // absolute db end (new) / unused (resolved)
  uint32_t query;     // candidate's own query (frame)
  int32_t from;       // -1: new candidate; else position in the group's old results
};
struct ScoreDesc {
  bool operator()(const MergeItem &a, const MergeItem &b) const { return a.score > b.score; }
};
}  // namespace

// reference Merge (aligner.cpp:687-769): per name group, the batch's candidates
// of each query then its kept results, std::sort by score (unstable), first hit
// per subject traced back, stop at -b. Groups are independent -> host threads.
// Used when a chunk needs several batches or several DB chunks.
void Session::HostMergeBatch(QueryData &q, DbData &d, uint32_t bq0, uint32_t bq1,
                             uint64_t cand_begin, const uint32_t *score, const uint32_t *end,
                             const std::vector<uint32_t> &counts, const std::vector<uint64_t> &offsets,
                             Results *results) {
  const uint32_t ng = (uint32_t)q.group_first.size();
  const uint64_t epoch = ++merge_epoch_;
  const uint32_t nsubj = d.chunk.nseq;
  struct Pending {
    uint32_t id, pos;
  };
  std::vector<std::vector<Pending>> pending(threads_);
  ParallelFor(ng, threads_, [&](size_t gb, size_t ge, unsigned t) {
    std::vector<uint64_t> owner(nsubj, ~0ull);
    std::vector<MergeItem> l;
    std::vector<HitRecord> old;
    for (size_t g = gb; g < ge; ++g) {
      const uint32_t gs = q.group_first[g], gend = q.group_last[g] + 1, id = gend - 1;
      l.clear();
      old.clear();
      for (uint32_t i = gs; i < gend; ++i) {
        if (i >= bq0 && i < bq1) {
          const uint64_t b = offsets[i] - cand_begin;
          for (uint32_t k = 0; k < counts[i]; ++k)
            l.push_back(MergeItem{score[b + k], end[b + k], i, -1});
        }
        for (HitRecord &h : (*results)[i]) {
          l.push_back(MergeItem{h.score, 0, h.query, (int32_t)old.size()});
          old.push_back(h);
        }
        (*results)[i].clear();
      }
      if (l.empty()) continue;
      std::sort(l.begin(), l.end(), ScoreDesc());
      std::vector<HitRecord> &out = (*results)[id];
      const uint64_t tag = (epoch << 32) | id;
      for (const MergeItem &it : l) {
        if (it.from >= 0) {
          out.push_back(old[it.from]);
        } else {
          const uint32_t sid = d.chunk.SubjectOf(it.end);
          if (sid >= nsubj) throw Error("candidate end outside the database");
          if (owner[sid] != tag) {
            owner[sid] = tag;
            HitRecord h;
            h.query = it.query;
            h.db_chunk = d.chunk.id;
            h.subject = sid;
            h.score = it.score;
            h.end = it.end;          // absolute until the traceback
            h.start = UINT32_MAX;
            pending[t].push_back(Pending{id, (uint32_t)out.size()});
            out.push_back(h);
          }
        }
        if (out.size() >= opt_.best) break;
      }
    }
  });

  // K3 for every newly selected hit of this batch, then rebase to the subject
  std::vector<Pending> all;
  for (auto &p : pending) all.insert(all.end(), p.begin(), p.end());
  const uint32_t nh = (uint32_t)all.size();
  if (nh == 0) return;
  std::vector<uint32_t> qid(nh), e(nh), st(nh), len(nh), mt(nh);
  std::vector<float> sid(nh);
  for (uint32_t k = 0; k < nh; ++k) {
    const HitRecord &h = (*results)[all[k].id][all[k].pos];
    qid[k] = h.query;
    e[k] = h.end;
  }
  const uint32_t tb_base = TbBase(q);
  DeviceModule::Get().TraceBack(q.dev, d.dev, nh, qid.data(), e.data(), tb_base, opt_.open_gap,
                                opt_.extend_gap, st.data(), len.data(), mt.data(), sid.data());
  stats_.tracebacks += nh;
  for (uint32_t k = 0; k < nh; ++k) {
    HitRecord &h = (*results)[all[k].id][all[k].pos];
    const uint32_t pos = d.chunk.starts[h.subject];
    h.start = st[k] - pos;
    h.end = h.end - pos;
    h.aln_len = len[k];
    h.aln_match = mt[k];
    h.seq_id = sid[k];
  }
}

// Device path, one pass per (DB chunk, batch): the chunk's groups are cut into
// segments of ~kSegmentCands of the batch's candidates (at group boundaries, so
// every group's candidates stay together as in the reference batch); per
// segment K2 -> K4 -> K3 run on the GPU. K4 merges each group's candidates with
// the result list carried from the earlier passes (the reference Merge over
// result_list, aligner.cpp:687-769, called for every batch of every DB chunk,
// aligner.cpp:118-174); in the final pass the segment's text is formatted by the
// background worker while the GPU works on the next one.
void Session::DevicePass(QueryData &q, DbData &d, const std::vector<uint32_t> &counts,
                         const std::vector<uint64_t> &offsets, uint32_t bq0, uint32_t bq1, uint64_t c_lo,
                         uint64_t c_hi, bool carry_in, bool final_pass) {
  DeviceModule &dev = DeviceModule::Get();
  GapConfig gap;
  gap.extend = opt_.extend;
  gap.log_region = opt_.log_region;
  gap.open = opt_.open_gap;
  gap.ext = opt_.extend_gap;
  const uint32_t base = q.chunk.L + 2 * opt_.extend + 2 * (1u << opt_.log_region);
  const uint32_t tb_base = TbBase(q);
  const uint32_t cap = std::max<uint32_t>(opt_.best, 1);
  // segments of ~16M candidates (fewer host round trips per step);
  // GHOSTM_SEGMENT_CANDS / GHOSTM_TAIL_CANDS shrink them so that small test
  // datasets run the many-segment pipeline of the full-size workloads
  // The tail floor is 1 M candidates, or a quarter of a smaller batch, so a
  // batch of under ~2 M candidates is still cut into three segments whose
  // formatting overlaps the next one's K2 (cfg2's 0.9 M: 10.2 -> 8.7 ms per
  // step; at cfg3 and the 125 K shard a smaller floor only adds launches,
  // profiles/r4_tail_sweep.txt)
  // The floor's cap counts the last segment's formatting, which grows with its
  // queries, not its candidates: 1 M candidates or 16 K queries' worth,
  // whichever is more (dense batches, 127 per query: ~2 M; cfg4 351.1 -> 350.5
  // ms, the 125 K shard 46.7 -> 46.4 ms; cfg3's 63 per query keeps ~1 M: 2 M
  // lost 0.5 ms there, profiles/r5aj/, profiles/r5ai/)
  const uint64_t batch_q = bq1 > bq0 ? bq1 - bq0 : 1;
  const uint64_t tail_cap = std::max<uint64_t>(1ull << 20, (c_hi - c_lo) / batch_q * 16384);
  uint64_t kSegmentCands = 16ull << 20;
  uint64_t kTailCands = std::min<uint64_t>(tail_cap, std::max<uint64_t>(1ull << 17, (c_hi - c_lo) / 4));
  if (const char *e = getenv("GHOSTM_SEGMENT_CANDS")) kSegmentCands = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
  if (const char *e = getenv("GHOSTM_TAIL_CANDS")) kTailCands = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
  // the first segment's K2 tasks are built while the GPU waits (the later
  // ones during the previous K2): a head of at most kHeadCands shortens that
  // wait (GHOSTM_HEAD_CANDS; 0 = no head cap). At >= 96 candidates per query the
  // unit kernel's consecutive tasks need no count pass (score_tasks.h) and the
  // build is short (0.04 ms for the 125 K-query shard's first 1 M): no head
  // there, one segment fewer (shard 46.5-46.8 against 46.7-47.5 ms with it,
  // profiles/r5t/)
  uint64_t kHeadCands = (c_hi - c_lo) / batch_q >= 96 ? 0 : kTailCands;
  if (const char *e = getenv("GHOSTM_HEAD_CANDS")) kHeadCands = strtoull(e, nullptr, 10);
  const uint32_t ng = (uint32_t)q.group_first.size();
  // a group's first candidate of this batch (groups outside it have none)
  auto group_begin = [&](uint32_t g) { return std::min(std::max(offsets[q.group_first[g]], c_lo), c_hi); };
  auto group_of = [&](uint32_t qi) {
    return (uint32_t)(std::upper_bound(q.group_first.begin(), q.group_first.end(), qi) - q.group_first.begin()) - 1;
  };
  // the batch's groups [gb0, gb1) (a batch may cut a name group); the groups
  // before and after it have no new candidates
  const uint32_t gb0 = bq1 > bq0 ? group_of(bq0) : 0, gb1 = bq1 > bq0 ? group_of(bq1 - 1) + 1 : 0;
  // segment cuts (group ranges) first, so each segment's K2 tasks can be built
  // on the host while the previous segment's K2 runs
  std::vector<std::pair<uint32_t, uint32_t>> cuts;
  const uint32_t kIdleGroups = 1u << 17;  // groups per segment without candidates
  auto idle = [&](uint32_t from, uint32_t to) {
    for (uint32_t g = from; g < to; g += kIdleGroups) cuts.emplace_back(g, std::min(to, g + kIdleGroups));
  };
  idle(0, gb0);
  for (uint32_t g0 = gb0; g0 < gb1;) {
    const uint64_t rem = c_hi - group_begin(g0);  // candidates from g0 to the batch's end
    // full segments, then shrinking ones (3/5 of what is left, down to
    // kTailCands): each segment's GPU time (~3.5 ms per 1 M candidates) covers
    // the text formatting of the one before it (~1.4 ms per 1 M), so little of
    // the formatting is left when the GPU finishes
    // (a carried pass formats nothing: full segments only)
    uint64_t target = rem > 2 * kSegmentCands || !final_pass ? kSegmentCands
                                                              : std::max<uint64_t>(kTailCands, rem * 3 / 5);
    if (g0 == gb0 && kHeadCands && rem > 2 * kHeadCands) target = std::min(target, kHeadCands);
    // the first group g1 > g0 at least `target` candidates on (group_begin
    // does not decrease with g: a binary search, not a walk over the groups)
    const uint64_t from = group_begin(g0);
    uint32_t lo = g0 + 1, hi = gb1;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (group_begin(mid) - from < target) lo = mid + 1;
      else hi = mid;
    }
    const uint32_t g1 = lo;
    cuts.emplace_back(g0, g1);
    g0 = g1;
  }
  idle(gb1, ng);
  TraceMark("cuts", cuts.size());
  std::vector<DeviceModule::ScoreSegment> segs;
  for (const auto &c : cuts) {
    const uint64_t c0 = group_begin(c.first), c1 = c.second < ng ? group_begin(c.second) : c_hi;
    segs.push_back({c0, c1 - c0, q.group_first[c.first], q.group_last[c.second - 1] + 1});
  }
  MergePass pass;
  pass.cand_lo = c_lo;
  pass.cand_hi = c_hi;
  pass.carry_in = carry_in;
  pass.carry_out = !final_pass;
  pass.chunk = d.chunk.id;
  // Pipeline, per segment k: K2(k) is enqueued first; then segment k-1's
  // selection (its K4/K3 finished before K2(k) started) is copied back on the
  // copy stream, turned into records and handed to the formatter while K2(k)
  // runs; then K4/K3(k) are enqueued behind K2(k) (after K2 finishes when its
  // guard list needs re-scoring first). The GPU never waits for the host
  // between segments.
  struct Pending {
    uint32_t g0 = 0, g1 = 0;
    bool active = false, identity = false;
  } pending;
  auto finish_pending = [&] {
    if (!pending.active) return;
    pending.active = false;
    const uint32_t g0 = pending.g0;
    auto sel_counts = std::make_shared<std::vector<uint32_t>>();
    auto sel_hits = std::make_shared<HostHits>();
    const double t0 = NowSeconds();
    dev.MergeCollect(sel_counts.get(), final_pass ? sel_hits.get() : nullptr);
    stats_.seconds_merge += NowSeconds() - t0;
    TraceMark("merge_done", pending.g1 - g0);
    if (!final_pass) return;
    dev.AppendRecords(q.dev, g0, *sel_counts, cap, q.global_base, false);
    Part *part = NewPart();
    const QueryData *qp = &q;
    TraceMark("records", g0);
    formatter_->Submit([this, qp, g0, sel_counts, sel_hits, cap, part] {
      const double t = NowSeconds();
      TraceMark("fmt_begin", g0);
      FormatSelected(*qp, g0, *sel_counts, *sel_hits, cap, part);
      stats_.seconds_output += NowSeconds() - t;
      TraceMark("fmt_end", g0);
      PartDone(part);
    });
  };
  struct DeferNext {  // ScorePrepareNext below builds each next segment's tasks
    DeviceModule &dev;
    explicit DeferNext(DeviceModule &d) : dev(d) { dev.ScoreDeferNext(true); }
    ~DeferNext() { dev.ScoreDeferNext(false); }
  } defer_next{dev};
  for (size_t k = 0; k < cuts.size(); ++k) {
    const uint32_t g0 = cuts[k].first, g1 = cuts[k].second;
    const uint64_t c0 = segs[k].cand_begin, c1 = c0 + segs[k].n;
    // nothing to merge: no candidates and nothing carried (the carry of these
    // groups is still the empty list ResetCarry left). Groups without new
    // candidates keep their carried list as it is when -b <= 16: it is sorted
    // by score, std::sort of <= 16 elements is a stable insertion sort, and
    // carried entries are all taken (aligner.cpp:719-721); in the final pass
    // their lists are printed straight from the carry
    const bool identity = c1 == c0 && carry_in && opt_.best <= 16;
    const bool work = c1 > c0 || (carry_in && !identity);
    TraceMark("seg", k);
    if (c1 > c0)
      dev.ScoreLaunch(q.dev, d.dev, c0, c1 - c0, segs[k].q_first, segs[k].q_end, counts, offsets, base, gap,
                      k + 1 < segs.size() ? &segs[k + 1] : nullptr);
    finish_pending();  // segment k - 1, while K2(k) runs
    const bool guarded = dev.ScoreGuarded();
    if (work && !guarded) {
      dev.MergeLaunch(q.dev, d.dev, g0, g1, c0, c1 - c0, opt_.best, tb_base, opt_.open_gap, opt_.extend_gap, pass);
      pending = Pending{g0, g1, true, false};
    }
    // segment k + 1's K2 tasks, while K2(k) and K4/K3(k) run
    dev.ScorePrepareNext(counts, offsets);
    dev.ScoreFinish();
    TraceMark("score_done", c1 - c0);
    if (work && guarded) {
      dev.MergeLaunch(q.dev, d.dev, g0, g1, c0, c1 - c0, opt_.best, tb_base, opt_.open_gap, opt_.extend_gap, pass);
      pending = Pending{g0, g1, true, false};
    }
    stats_.segments += 1;
    if (work || !final_pass) continue;
    // no K4 for these groups: their lists come straight from the carry (or are
    // empty), formatted in order behind the pending segment's
    finish_pending();
    auto sel_counts = std::make_shared<std::vector<uint32_t>>();
    auto sel_hits = std::make_shared<HostHits>();
    if (identity) {
      dev.CarryToHost(q.dev, g0, g1, cap, sel_counts.get(), sel_hits.get());
      dev.AppendRecords(q.dev, g0, *sel_counts, cap, q.global_base, true);
    } else {
      sel_counts->assign(g1 - g0, 0);
    }
    Part *part = NewPart();
    const QueryData *qp = &q;
    formatter_->Submit([this, qp, g0, sel_counts, sel_hits, cap, part] {
      const double t = NowSeconds();
      FormatSelected(*qp, g0, *sel_counts, *sel_hits, cap, part);
      stats_.seconds_output += NowSeconds() - t;
      PartDone(part);
    });
  }
  finish_pending();
}

void Session::RunQueryChunk(QueryData &q) {
  DeviceModule &dev = DeviceModule::Get();
  SeedConfig sc;
  sc.threshold = opt_.threshold;
  sc.shift = opt_.shift;
  sc.log_region = opt_.log_region;
  // K1's per-query counts and offsets: session buffers, reused by every chunk
  // and run (a fresh vector's zero-fill and first-touch faults sat before K1's
  // first kernel: 6 MB per cfg4 chunk)
  std::vector<uint32_t> &counts = seed_counts_;
  std::vector<uint64_t> &offsets = seed_offsets_;
  // the device merge needs every DB chunk's subject table; GHOSTM_MERGE=host
  // keeps the host merge (tests)
  bool device_merge = true;
  for (const DbData &d : dbs_) device_merge = device_merge && d.chunk.nseq > 0;
  if (const char *e = getenv("GHOSTM_MERGE")) device_merge = device_merge && strcmp(e, "host") != 0;
  if (!device_merge) {
    RunQueryChunkHostMerge(q);
    return;
  }
  const uint32_t cap = std::max<uint32_t>(opt_.best, 1);
  dev.ResetCarry(q.dev, cap);
  if (run_sync_) dev.Synchronize();  // (see Run)
  TraceMark("carry_idle");
  bool carry = false, formatted = false;
  for (size_t di = 0; di < dbs_.size(); ++di) {
    DbData &d = dbs_[di];
    sc.seed_mask = d.chunk.seed;
    TraceMark("seed", q.chunk.nseq);
    const uint64_t total = dev.Seed(q.dev, d.dev, sc, &counts, &offsets);
    stats_.candidates += total;
    TraceMark("seed_done", total);
    // (a shard replays the unsharded run's batches; those that miss its
    // queries are passes without candidates over its carried lists)
    const std::vector<Batch> batches = Passes(q, di, counts, total);
    TraceMark("batches", batches.size());
    for (size_t bi = 0; bi < batches.size(); ++bi) {
      const Batch &b = batches[bi];
      const uint64_t c0 = b.q0 < counts.size() ? offsets[b.q0] : total;
      const uint64_t c1 = b.q1 < counts.size() ? offsets[b.q1] : total;
      const bool final_pass = di + 1 == dbs_.size() && bi + 1 == batches.size();
      DevicePass(q, d, counts, offsets, b.q0, b.q1, c0, c1, carry, final_pass);
      carry = true;
      formatted = final_pass;
      stats_.batches += 1;
    }
  }
  if (!formatted) {
    // the last DB chunk had no batch: the carried lists are the results
    auto sel_counts = std::make_shared<std::vector<uint32_t>>();
    auto sel_hits = std::make_shared<HostHits>();
    dev.CarryToHost(q.dev, 0, (uint32_t)q.group_first.size(), cap, sel_counts.get(), sel_hits.get());
    records_on_device_ = false;  // records are uploaded from the host on demand
    Part *part = NewPart();
    const QueryData *qp = &q;
    formatter_->Submit([this, qp, sel_counts, sel_hits, cap, part] {
      const double t = NowSeconds();
      FormatSelected(*qp, 0, *sel_counts, *sel_hits, cap, part);
      stats_.seconds_output += NowSeconds() - t;
      PartDone(part);
    });
  }
}

// Host merge (GHOSTM_MERGE=host, or a DB chunk without subjects): every batch's
// scores come back to the host and HostMergeBatch applies the reference Merge.
void Session::RunQueryChunkHostMerge(QueryData &q) {
  DeviceModule &dev = DeviceModule::Get();
  SeedConfig sc;
  sc.threshold = opt_.threshold;
  sc.shift = opt_.shift;
  sc.log_region = opt_.log_region;
  GapConfig gap;
  gap.extend = opt_.extend;
  gap.log_region = opt_.log_region;
  gap.open = opt_.open_gap;
  gap.ext = opt_.extend_gap;
  const uint32_t base = q.chunk.L + 2 * opt_.extend + 2 * (1u << opt_.log_region);
  std::vector<uint32_t> counts;
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> score, end;
  Results results(q.chunk.nseq);
  records_on_device_ = false;  // host merge: records are uploaded on demand
  for (size_t di = 0; di < dbs_.size(); ++di) {
    DbData &d = dbs_[di];
    sc.seed_mask = d.chunk.seed;
    const uint64_t total = dev.Seed(q.dev, d.dev, sc, &counts, &offsets);
    stats_.candidates += total;
    const std::vector<Batch> batches = Passes(q, di, counts);
    TraceMark("batches", batches.size());
    for (const Batch &b : batches) {
      const uint64_t c0 = b.q0 < counts.size() ? offsets[b.q0] : total;
      const uint64_t c1 = b.q1 < counts.size() ? offsets[b.q1] : total;
      const uint64_t nc = c1 - c0;
      score.resize(nc);
      end.resize(nc);
      if (nc) dev.Score(q.dev, d.dev, c0, nc, b.q0, b.q1, counts, offsets, base, gap, score.data(), end.data());
      const double t0 = NowSeconds();
      HostMergeBatch(q, d, b.q0, b.q1, c0, score.data(), end.data(), counts, offsets, &results);
      stats_.seconds_merge += NowSeconds() - t0;
      stats_.batches += 1;
    }
  }
  formatter_->Drain();
  const double t1 = NowSeconds();
  Part *part = NewPart();
  FormatResults(q, results, part);
  PartDone(part);
  stats_.seconds_output += NowSeconds() - t1;
}

// ------------------------------------------------------------------ output
namespace {
// two-digit table for integer formatting
struct Digits {
  char d[200];
  Digits() {
    for (int i = 0; i < 100; ++i) { d[2 * i] = (char)('0' + i / 10); d[2 * i + 1] = (char)('0' + i % 10); }
  }
};
const Digits kDigits;

inline char *PutU32(char *p, uint32_t v) {
  char buf[12];
  char *e = buf + sizeof(buf), *b = e;
  while (v >= 100) {
    const uint32_t r = v % 100;
    v /= 100;
    b -= 2;
    std::memcpy(b, kDigits.d + 2 * r, 2);
  }
  if (v >= 10) {
    b -= 2;
    std::memcpy(b, kDigits.d + 2 * v, 2);
  } else {
    *--b = (char)('0' + v);
  }
  std::memcpy(p, b, (size_t)(e - b));
  return p + (e - b);
}
// ostream << float == printf("%g") == to_chars(general, 6) (checked on 6e8 bit
// patterns incl. NaN/inf/denormals), and to_chars is ~5x faster than snprintf.
inline char *PutFloat(char *p, float f) {
  return std::to_chars(p, p + 48, f, std::chars_format::general, 6).ptr;
}
inline char *PutStr(char *p, std::string_view s) {
  std::memcpy(p, s.data(), s.size());
  return p + s.size();
}
// %g text of at most 15 bytes (every float's fits: "-1.17549e-38" is 12)
inline char *PutFloat15(char *p, float f) {
  return std::to_chars(p, p + 15, f, std::chars_format::general, 6).ptr;
}
constexpr uint32_t kIdLen = 512, kIdMatch = 128;
}  // namespace

// A table of short texts (at most 15 bytes) filled on first use: entry = bytes
// 0..14 the text, byte 15 its length (0: not yet), in two 64-bit atomics (the
// second, holding the length, published last); racing writers store the same
// bytes. A hit copies the 16 bytes straight from the two loaded words into the
// line (which has kFixed bytes of room) and steps on by the length: no reload
// from a stack buffer at an odd offset, which stalled on store forwarding. The
// storage comes zeroed from calloc (the OS's zero pages), so a table costs
// nothing until entries are used: the session's create -> run path no longer
// formats 60 K identity strings up front.
struct TextCache {
  struct Entry {
    std::atomic<uint64_t> a, b;
  };
  Entry *e = nullptr;
  size_t n = 0;
  explicit TextCache(size_t entries) : e(static_cast<Entry *>(std::calloc(entries, sizeof(Entry)))), n(entries) {
    if (!e) throw std::bad_alloc();
  }
  ~TextCache() { std::free(e); }
  TextCache(const TextCache &) = delete;
  TextCache &operator=(const TextCache &) = delete;
  // the text of entry k, made by make(buf) (writes at most 15 bytes, returns its end) on first use
  template <class F>
  char *Put(char *p, size_t k, F make) const {
    Entry &c = e[k];
    uint64_t w[2];
    w[1] = c.b.load(std::memory_order_acquire);
    if ((w[1] >> 56) == 0) {
      char buf[16] = {0};
      buf[15] = (char)(make(buf) - buf);
      std::memcpy(w, buf, 16);
      c.a.store(w[0], std::memory_order_relaxed);
      c.b.store(w[1], std::memory_order_release);
    } else {
      w[0] = c.a.load(std::memory_order_relaxed);
    }
    std::memcpy(p, w, 16);
    return p + (w[1] >> 56);
  }
};

// One output line, WriteOutput / V1 / V2 (aligner.cpp:951-1012). Everything that
// depends only on the score (bits, exp(-lambda*s)), only on (len, matches) (the
// identity) or only on (query length, score) (the E-value: search space = qlen x
// the DB's residue sum) is formatted once per session, by whichever formatter
// thread needs it first (TextCache); the arithmetic is the reference's float /
// double steps.
struct LineFormat {
  int style = 0;
  EvalueCalculator ev;
  std::vector<double> expd;           // per score: exp(-1.0 * s * lambda)
  static constexpr uint32_t kEvScores = 4096;
  std::unique_ptr<TextCache> bits_txt;  // per score
  std::unique_ptr<TextCache> id_txt;    // per (len, match): 100*id (style 0) or id (style 2)
  std::unique_ptr<TextCache> ev_txt;    // per (query length, score)

  LineFormat(int st, const KarlinParams &k, uint32_t max_score) : style(st), ev(k) {
    if (style == 0) {
      expd.resize(max_score + 1);
      for (uint32_t sc = 0; sc <= max_score; ++sc) expd[sc] = exp(static_cast<double>(-1.0 * (int)sc * ev.p.lambda));
      bits_txt.reset(new TextCache(max_score + 1));
      ev_txt.reset(new TextCache((size_t)(kMaxQueryLength + 1) * kEvScores));
    }
    if (style != 1) id_txt.reset(new TextCache((size_t)kIdLen * kIdMatch));
  }
  float Id(uint32_t len, uint32_t m) const {
    const float id = (float)m / (float)len;  // aligner.cpp:945
    return style == 0 ? id * 100 : id;
  }
  char *PutId(char *p, uint32_t len, uint32_t m) const {
    if (len < kIdLen && m < kIdMatch && m <= len && len > 0)
      return id_txt->Put(p, (size_t)len * kIdMatch + m, [&](char *b) { return PutFloat15(b, Id(len, m)); });
    return PutFloat(p, Id(len, m));
  }
  // the E-value (float)((double)scaled * exp(-lambda * score)), as %g text
  char *PutEvalue(char *p, uint32_t qlen, uint32_t score, float scaled) const {
    const double e = score < expd.size() ? expd[score] : exp(static_cast<double>(-1.0 * (int)score * ev.p.lambda));
    if (qlen > kMaxQueryLength || score >= kEvScores || !ev_txt) return PutFloat(p, (float)((double)scaled * e));
    return ev_txt->Put(p, (size_t)qlen * kEvScores + score, [&](char *b) { return PutFloat15(b, (float)((double)scaled * e)); });
  }
  char *PutBits(char *p, uint32_t score) const {
    if (bits_txt && score < bits_txt->n)
      return bits_txt->Put(p, score, [&](char *b) { return PutFloat15(b, ev.Bits((int)score)); });
    return PutFloat(p, ev.Bits((int)score));
  }
  // bytes a line can take beyond the two names
  static constexpr size_t kFixed = 160;
  // scaled = (float)search_space * K, per query of non-X length qlen
  char *Write(char *p, std::string_view qname, std::string_view sname, uint32_t score, uint32_t start,
              uint32_t end, uint32_t len, uint32_t match, float scaled, uint32_t qlen) const {
    p = PutStr(p, qname);
    *p++ = '\t';
    p = PutStr(p, sname);
    *p++ = '\t';
    if (style == 1) {
      p = PutU32(p, score); *p++ = '\t';
      p = PutU32(p, start + 1); *p++ = '\t';
      p = PutU32(p, end + 1);
    } else if (style == 2) {
      p = PutU32(p, score); *p++ = '\t';
      p = PutU32(p, start + 1); *p++ = '\t';
      p = PutU32(p, end + 1); *p++ = '\t';
      p = PutId(p, len, match); *p++ = '\t';
      p = PutU32(p, len); *p++ = '\t';
      p = PutU32(p, match);
    } else {
      p = PutId(p, len, match); *p++ = '\t';
      p = PutU32(p, len); *p++ = '\t';
      p = PutU32(p, match); *p++ = '\t';
      p = PutU32(p, start + 1); *p++ = '\t';
      p = PutU32(p, end + 1); *p++ = '\t';
      p = PutEvalue(p, qlen, score, scaled); *p++ = '\t';
      p = PutBits(p, score); *p++ = '\t';
    }
    *p++ = '\n';
    return p;
  }
};

namespace {
// Appends lines through a raw cursor into a std::string that grows in chunks.
struct TextCursor {
  std::string &s;
  size_t used;
  explicit TextCursor(std::string &str) : s(str), used(str.size()) {}
  char *Reserve(size_t need) {
    if (s.size() < used + need) s.resize(std::max(used + need, s.size() * 2 + 4096));
    return &s[used];
  }
  void Commit(char *end) { used = (size_t)(end - s.data()); }
  ~TextCursor() { s.resize(used); }
};
}  // namespace

// pieces per formatting worker in a streamed run (GHOSTM_STREAM_PIECES, A/B;
// 1 = the part's pieces as in a run without a file)
static size_t StreamPiecesPerWorker() {
  static const size_t v = [] {
    const char *e = getenv("GHOSTM_STREAM_PIECES");
    return e ? (size_t)std::max(1, atoi(e)) : (size_t)4;
  }();
  return v;
}

const LineFormat &Session::Format() {
  // -y 6 formats style-0 lines first: FormatTabular takes their identity,
  // E-value and bit-score bytes
  const bool tabular =
      (opt_.output_style >= 6 && opt_.output_style <= 9) || (opt_.output_style >= 12 && opt_.output_style <= 15) ||
      opt_.output_style == 20 || opt_.output_style == 21;
  // -y 10, -y 11 and -y 16 to -y 19 replace the hit lines after the run: style 1's lines, which need no E-value, stand in
  const bool pileup = opt_.output_style == 10 || opt_.output_style == 11 || (opt_.output_style >= 16 && opt_.output_style <= 19) ||
                      (opt_.output_style >= 22 && opt_.output_style <= 27);  // and the taxon lines, the profile, the pairs
  if (!format_) format_.reset(new LineFormat(tabular ? 0 : pileup ? 1 : opt_.output_style, opt_.karlin, 4095));
  return *format_;
}

// What a pass added to the device's counters: dst.*to += after.*from - before.*from
// for every (to, from) pair of members.
template <class Dst, class... To, class... From>
static void AddDeltas(Dst &dst, const DeviceTimes &before, const DeviceTimes &after,
                      std::pair<To Dst::*, From DeviceTimes::*>... m) {
  ((dst.*m.first += after.*m.second - before.*m.second), ...);
}

// The read-level passes' counters (DeviceTimes holds them as the public structs)
// are added whole: every one of the seven structs is one double, the seconds,
// followed by uint64_t counters only.
template <class Stats, size_t kFields>
constexpr bool SecondsThenCounters(double Stats::*) {
  return std::is_trivially_copyable<Stats>::value && sizeof(Stats) == 8 * kFields;
}
static_assert(SecondsThenCounters<GhostmBandStats, 5>(&GhostmBandStats::seconds_band) &&
                  SecondsThenCounters<GhostmFrameStats, 5>(&GhostmFrameStats::seconds_frame) &&
                  SecondsThenCounters<GhostmReadRowsStats, 4>(&GhostmReadRowsStats::seconds_read_rows) &&
                  SecondsThenCounters<GhostmReadPileupStats, 6>(&GhostmReadPileupStats::seconds_read_pileup) &&
                  SecondsThenCounters<GhostmReadCullStats, 7>(&GhostmReadCullStats::seconds_cull) &&
                  SecondsThenCounters<GhostmReadLcaStats, 6>(&GhostmReadLcaStats::seconds_lca) &&
                  SecondsThenCounters<GhostmTaxonProfileStats, 4>(&GhostmTaxonProfileStats::seconds_profile) &&
                  SecondsThenCounters<GhostmPairJoinStats, 6>(&GhostmPairJoinStats::seconds_pair),
              "a pass's counters: a double, then 8-byte counters");
static_assert(offsetof(GhostmBandStats, seconds_band) == 0 && offsetof(GhostmFrameStats, seconds_frame) == 0 &&
                  offsetof(GhostmReadRowsStats, seconds_read_rows) == 0 &&
                  offsetof(GhostmReadPileupStats, seconds_read_pileup) == 0 &&
                  offsetof(GhostmReadCullStats, seconds_cull) == 0 && offsetof(GhostmReadLcaStats, seconds_lca) == 0 &&
                  offsetof(GhostmTaxonProfileStats, seconds_profile) == 0,
              "a pass's counters begin with the seconds");

// dst += x (or dst -= x), field by field
template <class Stats>
static void AddStats(Stats &dst, const Stats &x, bool subtract = false) {
  constexpr size_t n = sizeof(Stats) / 8;
  uint64_t d[n], v[n];
  double ds, vs;
  memcpy(d, &dst, sizeof(Stats));
  memcpy(v, &x, sizeof(Stats));
  memcpy(&ds, d, 8);
  memcpy(&vs, v, 8);
  ds = subtract ? ds - vs : ds + vs;
  memcpy(d, &ds, 8);
  for (size_t k = 1; k < n; ++k) d[k] = subtract ? d[k] - v[k] : d[k] + v[k];
  memcpy(&dst, d, sizeof(Stats));
}

// What a pass added to its counters: after - before
template <class Stats>
static Stats StatsDelta(Stats after, const Stats &before) {
  AddStats(after, before, true);
  return after;
}

// The index of the tile at `offset` within its source of m letters and `tiles`
// tiles (query_tiles.h: the last tile ends with the source).
static uint32_t TileIndex(uint32_t offset, uint32_t tiles, uint32_t m, uint32_t W, uint32_t step) {
  return offset == TileStart(tiles - 1, tiles, m, W, step) ? tiles - 1 : offset / step;
}

uint32_t Session::TbBase(const QueryData &q) const {
  return q.chunk.L + 2 * opt_.extend * 2 * (1u << opt_.log_region);
}

std::vector<std::vector<size_t>> Session::HitsByChunkPair() const {
  std::vector<std::vector<size_t>> groups(queries_.size() * dbs_.size());
  for (size_t h = 0; h < hit_source_.size(); ++h)
    groups[hit_source_[h].qi * dbs_.size() + hit_source_[h].di].push_back(h);
  return groups;
}

template <class Item, class F> void Session::ForChunkPairs(const std::vector<std::vector<Item>> &groups, F fn) {
  for (size_t qi = 0; qi < queries_.size(); ++qi)
    for (size_t di = 0; di < dbs_.size(); ++di)
      if (!groups[qi * dbs_.size() + di].empty()) fn(qi, di, groups[qi * dbs_.size() + di]);
}

// The words in hit order: hit h's words leave its chunk pair's words[qi *
// dbs_.size() + di], where (*path)[h].ops_offset still points, for *ops.
void Session::JoinWords(const std::vector<std::vector<uint32_t>> &words, std::vector<GhostmHitPath> *path,
                        std::vector<uint32_t> *ops) const {
  for (size_t h = 0; h < path->size(); ++h) {
    GhostmHitPath &p = (*path)[h];
    const std::vector<uint32_t> &w = words[hit_source_[h].qi * dbs_.size() + hit_source_[h].di];
    const size_t at = ops->size();
    ops->insert(ops->end(), w.begin() + p.ops_offset, w.begin() + p.ops_offset + p.n_runs);
    p.ops_offset = at;
  }
}

// The rows passes' plan (HitsRows, HitsReadRows): the hits' column counts give
// every hit its place in hit order and *bytes its size; then per (query chunk,
// DB chunk) call(qi, di, items, rec, dst) with the items' paths, their subject
// coordinates absolute in the chunk again, and their places.
template <class Call>
void Session::RowsPlan(const std::vector<GhostmHitPath> &path, const std::vector<uint32_t> &words,
                       std::vector<uint8_t> *bytes, Call call) {
  const std::vector<GhostmHit> &hits = Hits();
  std::vector<uint64_t> place(hits.size());
  uint64_t total = 0;
  for (size_t h = 0; h < hits.size(); ++h) {
    uint64_t cols = 0;
    for (uint32_t r = 0; r < path[h].n_runs; ++r) cols += words[path[h].ops_offset + r] >> 4;
    place[h] = total;
    total += 3 * cols;
  }
  bytes->assign(total, 0);
  std::vector<uint64_t> dst;
  std::vector<GhostmHitPath> rec;
  ForChunkPairs(HitsByChunkPair(), [&](size_t qi, size_t di, const std::vector<size_t> &items) {
    dst.clear();
    rec.clear();
    for (size_t h : items) {
      GhostmHitPath p = path[h];
      const uint32_t pos = dbs_[di].chunk.starts[hits[h].db_id - dbs_[di].global_base];
      p.s_start += pos;
      p.s_end += pos;
      dst.push_back(place[h]);
      rec.push_back(p);
    }
    call(qi, di, items, rec, dst);
  });
}

template <class Extra, class Line> void Session::RewriteLines(const char *what, int tabs, Extra extra, Line line) {
  struct Piece {
    std::string *text;
    size_t first, n;
  };
  std::vector<Piece> pieces;
  size_t at = 0;
  for (size_t k = 0; k < used_parts_; ++k)
    for (size_t t = 0; t < parts_[k].text.size(); ++t) {
      pieces.push_back(Piece{&parts_[k].text[t], at, parts_[k].hits[t].size()});
      at += parts_[k].hits[t].size();
    }
  ParallelFor(pieces.size(), threads_, [&](size_t b, size_t e, unsigned) {
    std::string out;
    for (size_t pi = b; pi < e; ++pi) {
      const std::string &in = *pieces[pi].text;
      out.clear();
      out.reserve(in.size() + extra(pieces[pi].first, pieces[pi].n));
      size_t pos = 0, tab[8];
      for (size_t i = 0; i < pieces[pi].n; ++i) {
        const size_t nl = in.find('\n', pos);
        if (nl == std::string::npos) throw Error(std::string(what) + ": fewer lines than hits");
        size_t at_tab = nl;
        for (int c = 0; c < tabs; ++c) {
          if (at_tab <= pos) throw Error(std::string(what) + ": malformed line");
          at_tab = in.rfind('\t', at_tab - 1);
          if (at_tab == std::string::npos || at_tab < pos) throw Error(std::string(what) + ": malformed line");
          tab[c] = at_tab;
        }
        line(pieces[pi].first + i, in, pos, nl, tab, out);
        pos = nl + 1;
      }
      *pieces[pi].text = out;
    }
  });
  joined_valid_ = false;
}

// The extended traceback of every final hit (HitsExt). A hit names its query
// chunk and DB chunk through its global indices; its chunk-local query, its
// absolute end and its known start go to one TraceBackExt call per (query
// chunk, DB chunk). A hit record carries the last query of its name group (the
// reference's result_list[last]), not the query that scored: for a group of
// several queries (a DNA read's frames) every query of the group is traced and
// the first that reproduces the hit's (db_start, aln_len, aln_match) is taken.
const std::vector<GhostmHitExt> &Session::HitsExt() {
  if (hits_ext_valid_) return hits_ext_;
  formatter_->Drain();
  const std::vector<GhostmHit> &hits = Hits();
  hits_ext_.assign(hits.size(), GhostmHitExt{0, 0, 0, 0});
  hit_source_.assign(hits.size(), HitSource{0, 0, 0, 0, 0});
  struct Item {
    size_t hit;
    uint32_t q0, q1, end, start;  // queries [q0, q1] of the chunk; absolute DB coordinates
  };
  std::vector<std::vector<Item>> groups(queries_.size() * dbs_.size());
  for (size_t h = 0; h < hits.size(); ++h) {
    const GhostmHit &r = hits[h];
    size_t qi = 0, di = 0;
    while (qi < queries_.size() &&
           !(r.query_id >= queries_[qi].global_base && r.query_id - queries_[qi].global_base < queries_[qi].chunk.nseq))
      ++qi;
    while (di < dbs_.size() &&
           !(r.db_id >= dbs_[di].global_base && r.db_id - dbs_[di].global_base < dbs_[di].chunk.nseq))
      ++di;
    if (qi == queries_.size() || di == dbs_.size()) throw Error("extended traceback: hit outside the loaded chunks");
    const QueryData &q = queries_[qi];
    const uint32_t local = r.query_id - q.global_base;
    const size_t g = (size_t)(std::lower_bound(q.group_last.begin(), q.group_last.end(), local) - q.group_last.begin());
    uint32_t q0 = local, q1 = local;
    if (g < q.group_last.size() && q.group_first[g] <= local) q0 = q.group_first[g], q1 = q.group_last[g];
    const uint32_t pos = dbs_[di].chunk.starts[r.db_id - dbs_[di].global_base];
    groups[qi * dbs_.size() + di].push_back(Item{h, q0, q1, pos + r.db_end, pos + r.db_start});
  }
  DeviceModule &dev = DeviceModule::Get();
  const DeviceTimes before = dev.times();
  std::vector<uint32_t> qid, end, start_in, start, len, match;
  std::vector<GhostmHitExt> ext;
  ForChunkPairs(groups, [&](size_t qi, size_t di, const std::vector<Item> &items) {
    qid.clear();
    end.clear();
    start_in.clear();
    for (const Item &it : items)
      for (uint32_t f = it.q0; f <= it.q1; ++f) {
        qid.push_back(f);
        end.push_back(it.end);
        start_in.push_back(it.start);
      }
    const uint32_t n = (uint32_t)qid.size();
    start.resize(n);
    len.resize(n);
    match.resize(n);
    ext.resize(n);
    const QueryData &q = queries_[qi];
    dev.TraceBackExt(q.dev, dbs_[di].dev, n, qid.data(), end.data(), start_in.data(), TbBase(q), opt_.open_gap,
                     opt_.extend_gap, start.data(), len.data(), match.data(), ext.data());
    size_t k = 0;
    for (const Item &it : items) {
      const GhostmHit &r = hits[it.hit];
      bool found = false;
      for (uint32_t f = it.q0; f <= it.q1; ++f, ++k) {
        if (found || start[k] != it.start || len[k] != r.aln_len || match[k] != r.aln_match) continue;
        hits_ext_[it.hit] = ext[k];
        hit_source_[it.hit] = HitSource{(uint32_t)qi, (uint32_t)di, f, it.end, it.start};
        found = true;
      }
      if (!found) throw Error("extended traceback: no query of the hit's name group reproduces its alignment");
    }
  });
  AddDeltas(stats_, before, dev.times(), std::make_pair(&GhostmStats::seconds_traceback_ext, &DeviceTimes::traceback_ext),
            std::make_pair(&GhostmStats::traceback_ext_launches, &DeviceTimes::traceback_ext_launches),
            std::make_pair(&GhostmStats::traceback_ext_cells, &DeviceTimes::traceback_ext_cells));
  hits_ext_valid_ = true;
  return hits_ext_;
}

// The alignment path of every final hit (HitsPath): each hit's chunk-local
// query, absolute end and start as HitsExt() resolved them, one TraceBackPath
// call per (query chunk, DB chunk); the subject coordinates are made relative
// to the subject and the chunks' words joined in hit order.
const std::vector<GhostmHitPath> &Session::HitsPath() {
  if (hits_path_valid_) return hits_path_;
  HitsExt();
  const std::vector<GhostmHit> &hits = Hits();
  hits_path_.assign(hits.size(), GhostmHitPath{0, 0, 0, 0, 0, 0, 0});
  path_ops_.clear();
  const std::vector<std::vector<size_t>> groups = HitsByChunkPair();
  DeviceModule &dev = DeviceModule::Get();
  const DeviceTimes before = dev.times();
  std::vector<uint32_t> qid, end, start_in;
  std::vector<GhostmHitPath> rec;
  std::vector<std::vector<uint32_t>> words(groups.size());
  ForChunkPairs(groups, [&](size_t qi, size_t di, const std::vector<size_t> &items) {
    qid.clear();
    end.clear();
    start_in.clear();
    for (size_t h : items) {
      qid.push_back(hit_source_[h].query);
      end.push_back(hit_source_[h].end);
      start_in.push_back(hit_source_[h].start);
    }
    const uint32_t n = (uint32_t)items.size();
    rec.resize(n);
    const QueryData &q = queries_[qi];
    dev.TraceBackPath(q.dev, dbs_[di].dev, n, qid.data(), end.data(), start_in.data(), TbBase(q), opt_.open_gap,
                      opt_.extend_gap, rec.data(), &words[qi * dbs_.size() + di]);
    for (uint32_t k = 0; k < n; ++k) {
      const GhostmHit &r = hits[items[k]];
      const uint32_t pos = dbs_[di].chunk.starts[r.db_id - dbs_[di].global_base];
      GhostmHitPath p = rec[k];
      if (p.s_start != hit_source_[items[k]].start)
        throw Error("path traceback: a path does not begin at its hit's start");
      p.s_start -= pos;
      p.s_end -= pos;
      hits_path_[items[k]] = p;  // ops_offset: still within the chunk pair's words
    }
  });
  JoinWords(words, &hits_path_, &path_ops_);
  AddDeltas(stats_, before, dev.times(),
            std::make_pair(&GhostmStats::seconds_traceback_path, &DeviceTimes::traceback_path),
            std::make_pair(&GhostmStats::traceback_path_launches, &DeviceTimes::traceback_path_launches),
            std::make_pair(&GhostmStats::traceback_path_cells, &DeviceTimes::traceback_path_cells),
            std::make_pair(&GhostmStats::traceback_path_dir_bytes, &DeviceTimes::traceback_path_dir_bytes));
  hits_path_valid_ = true;
  return hits_path_;
}

const std::vector<uint32_t> &Session::PathOps() {
  HitsPath();
  return path_ops_;
}

// -y 7: the -y 6 columns with pident, length, mismatch, gapopen, qstart, qend,
// sstart and send taken from the hit's path (so a line agrees with itself), and
// a thirteenth column, the extended CIGAR. From the style-0 line: the two
// names, then the E-value and bit-score bytes; the fields are found from the
// line's end as in FormatTabular.
//
// -y 12 (read_level): a hit whose read-level score (HitsBand) is above 0 takes
// the eight columns and the CIGAR from its read-level path instead, in read or
// frame coordinates, and its E-value and bit score from the read-level score,
// priced like any line of the session for a query of the source's m letters
// (search space m x the database's residues; LineFormat's uncached branches
// take m > 127 and scores from 4096). A hit of read-level score 0 keeps its
// -y 7 line.
void Session::FormatPathTabular(bool read_level) {
  const std::vector<GhostmHitPath> &tile_path = HitsPath();
  const ReadLevelResult *lvl = read_level ? &ReadLevel(false) : nullptr;
  const LineFormat &w = Format();
  // tab[7]: the tab after the subject name
  RewriteLines("tabular output", 8, [](size_t, size_t n) { return n * 64; },
               [&](size_t hit, const std::string &in, size_t pos, size_t, const size_t *tab, std::string &out) {
    const bool band = lvl && lvl->rec[hit].score > 0;
    const GhostmHitPath &x = band ? lvl->rec[hit] : tile_path[hit];
    const std::vector<uint32_t> &ops = band ? lvl->ops : path_ops_;
    uint32_t count[4] = {0, 0, 0, 0}, gap_runs = 0;
    for (uint32_t r = 0; r < x.n_runs; ++r) {
      const uint32_t word = ops[x.ops_offset + r];
      count[word & 3u] += word >> 4;
      gap_runs += (word & 3u) >= 2;
    }
    const uint32_t length = count[0] + count[1] + count[2] + count[3];
    out.append(in, pos, tab[7] + 1 - pos);
    char num[160], *p = num;
    p = w.PutId(p, length, count[0]); *p++ = '\t';
    p = PutU32(p, length); *p++ = '\t';
    p = PutU32(p, count[1]); *p++ = '\t';
    p = PutU32(p, gap_runs); *p++ = '\t';
    const uint32_t q0 = (band ? 0u : TileOffset(hit)) + 1;  // a tiled set prints read coordinates
    p = PutU32(p, x.q_start + q0); *p++ = '\t';
    p = PutU32(p, x.q_end + q0); *p++ = '\t';
    p = PutU32(p, x.s_start + 1); *p++ = '\t';
    p = PutU32(p, x.s_end + 1); *p++ = '\t';
    if (band) {
      const uint32_t m = lvl->src[hit].letters;
      const float scaled = (float)((uint64_t)m * (uint64_t)db_sum_u32_) * w.ev.p.K;
      p = w.PutEvalue(p, m, x.score, scaled); *p++ = '\t';
      p = w.PutBits(p, x.score);
      out.append(num, (size_t)(p - num));
    } else {
      out.append(num, (size_t)(p - num));
      out.append(in, tab[2] + 1, tab[0] - tab[2] - 1);
    }
    out.push_back('\t');
    for (uint32_t r = 0; r < x.n_runs; ++r) {
      const uint32_t word = ops[x.ops_offset + r];
      p = PutU32(num, word >> 4);
      *p++ = "=XID"[word & 3u];
      out.append(num, (size_t)(p - num));
    }
    out.push_back('\n');
  });
}

// The aligned rows of every final hit (HitsRows): the hits' column counts give
// every hit its place in hit order, then one PathRows call per (query chunk, DB
// chunk) writes the bytes there; the paths' subject coordinates are made
// absolute in the chunk again.
const std::vector<GhostmHitRows> &Session::HitsRows() {
  if (hits_rows_valid_) return hits_rows_;
  const std::vector<GhostmHitPath> &path = HitsPath();
  hits_rows_.assign(Hits().size(), GhostmHitRows{0, 0, 0, 0, 0, 0, 0});
  DeviceModule &dev = DeviceModule::Get();
  const DeviceTimes before = dev.times();
  std::vector<uint32_t> qid;
  std::vector<GhostmHitRows> out;
  RowsPlan(path, path_ops_, &row_bytes_, [&](size_t qi, size_t di, const std::vector<size_t> &items,
                                             const std::vector<GhostmHitPath> &rec, const std::vector<uint64_t> &dst) {
    qid.clear();
    for (size_t h : items) qid.push_back(hit_source_[h].query);
    out.resize(items.size());
    dev.PathRows(queries_[qi].dev, dbs_[di].dev, (uint32_t)items.size(), qid.data(), rec.data(), path_ops_.data(),
                 path_ops_.size(), opt_.open_gap, opt_.extend_gap, queries_[qi].global_base, out.data(),
                 row_bytes_.data(), row_bytes_.size(), dst.data());
    for (size_t k = 0; k < items.size(); ++k) hits_rows_[items[k]] = out[k];
  });
  AddDeltas(stats_, before, dev.times(), std::make_pair(&GhostmStats::seconds_path_rows, &DeviceTimes::path_rows),
            std::make_pair(&GhostmStats::path_rows_launches, &DeviceTimes::path_rows_launches),
            std::make_pair(&GhostmStats::path_rows_columns, &DeviceTimes::path_rows_columns),
            std::make_pair(&GhostmStats::path_rows_bytes, &DeviceTimes::path_rows_bytes));
  hits_rows_valid_ = true;
  return hits_rows_;
}

const std::vector<uint8_t> &Session::RowBytes() {
  HitsRows();
  return row_bytes_;
}

void Session::SetBand(uint32_t band) {
  if (band < 1 || band > kBandMax) throw Error("band: half-width " + std::to_string(band) + " outside 1..31");
  if (band == band_) return;
  band_ = band;
  DropLevel(0);
  DropLevel(1);  // the frame pass runs inside the same band
}

void Session::SetFrameShift(int shift) {
  if (shift > 0 || shift < kFrameShiftMin)
    throw Error("shift: frameshift cost " + std::to_string(shift) + " outside -(1 << 20)..0");
  if (shift == frame_shift_) return;
  frame_shift_ = shift;
  DropLevel(1);
}

// A level's paths, or from its cull or its LCA on, and everything made from them
void Session::DropLevel(int lv, LevelStage from) {
  if (from == kFromPaths) {
    level_[lv].Drop();
    if (lv == 1) frame_info_.clear();
    read_rows_[lv].Drop();
    pileup_[kBandLevel + lv].Drop();
  }
  if (from != kFromLca) cull_[lv].Drop();
  lca_[lv].Drop();
  pair_[lv].Drop();  // made from the cull's records and the taxonomy's nodes
  pair_lca_[lv].Drop();
  profile_[lv].Drop();
}

// The read-level path of every final hit: the band paths (HitsBand) or the
// frame paths (HitsFrame). The record HitsExt() resolved for a hit is a tile of
// its source: the tile table gives the source's letters and the tile's offset,
// from which the tile's index and the source's first record follow (a protein
// record's tiles are consecutive records, a DNA frame's lie six records apart).
// On an untiled set every record is its own single-tile source. The frame
// pass's source is the strand of the tile's frame f: strand f / 3, beginning
// f % 3 records before the frame's own first record (the six frames of a tile
// are consecutive records). Both passes' anchor is the first cell of the tile
// path, on the frame level a codon diagonal. One BandAlign or FrameAlign call
// per (query chunk, DB chunk).
const Session::ReadLevelResult &Session::ReadLevel(bool frame) {
  ReadLevelResult &res = level_[frame ? 1 : 0];
  if (res.valid) return res;
  const std::string what = frame ? "frame align: " : "band align: ";
  if (frame && (tile_table_.empty() || !tile_dna_))
    throw Error(what + "the query set is not a DNA set made by a tiled setter");
  const std::vector<GhostmHitPath> &path = HitsPath();
  const std::vector<GhostmHit> &hits = Hits();
  res.rec.assign(hits.size(), GhostmHitPath{0, 0, 0, 0, 0, 0, 0});
  res.src.assign(hits.size(), GhostmBandSource{0, 0, 0, 0});
  res.ops.clear();
  if (frame) frame_info_.assign(hits.size(), GhostmHitFrameInfo{0, 0, 0, 0});
  const std::vector<std::vector<size_t>> groups = HitsByChunkPair();
  DeviceModule &dev = DeviceModule::Get();
  const DeviceTimes before = dev.times();
  std::vector<GhostmBandSource> src;
  std::vector<int32_t> diag;
  std::vector<uint32_t> lo, hi;
  std::vector<GhostmHitPath> rec;
  std::vector<std::vector<uint32_t>> words(groups.size());
  ForChunkPairs(groups, [&](size_t qi, size_t di, const std::vector<size_t> &items) {
    const QueryData &q = queries_[qi];
    const DbData &d = dbs_[di];
    const uint32_t W = q.chunk.L, step = tile_step_ ? tile_step_ : W;
    src.clear();
    diag.clear();
    lo.clear();
    hi.clear();
    for (size_t h : items) {
      const uint32_t local = hit_source_[h].query;
      GhostmBandSource s{local, 1, 1, q.qlen[local]};
      uint32_t offset = 0;
      if (!tile_table_.empty()) {
        const GhostmQueryTile &t = tile_table_[q.global_base + local];
        const uint32_t m = std::max(t.letters, 1u), tiles = TileCount(m, W, step);
        offset = t.offset;
        const uint32_t index = TileIndex(offset, tiles, m, W, step);
        const uint32_t stride = tile_dna_ ? 6u : 1u;
        const uint64_t back = (uint64_t)index * stride + (frame ? t.frame % 3 : 0u);
        if (back > local) throw Error(what + "a tile before its chunk's first record");
        s = GhostmBandSource{local - (uint32_t)back, stride, tiles, m};
        if (frame) frame_info_[h] = GhostmHitFrameInfo{t.frame / 3, tile_read_nt_[t.record], m, 0};
      }
      const uint32_t subject = hits[h].db_id - d.global_base, pos = d.chunk.starts[subject];
      src.push_back(s);
      // the first cell of the tile path, in source coordinates
      diag.push_back((int32_t)((int64_t)pos + path[h].s_start - ((int64_t)offset + path[h].q_start)));
      lo.push_back(pos);
      hi.push_back(pos + SubjectLength(d, subject) - 1);
    }
    const uint32_t n = (uint32_t)items.size();
    rec.resize(n);
    std::vector<uint32_t> *ops = &words[qi * dbs_.size() + di];
    if (frame)
      dev.FrameAlign(q.dev, d.dev, n, src.data(), diag.data(), lo.data(), hi.data(), step, band_, opt_.open_gap,
                     opt_.extend_gap, frame_shift_, rec.data(), ops);
    else
      dev.BandAlign(q.dev, d.dev, n, src.data(), diag.data(), lo.data(), hi.data(), step, band_, opt_.open_gap,
                    opt_.extend_gap, rec.data(), ops);
    for (uint32_t k = 0; k < n; ++k) {
      GhostmHitPath p = rec[k];
      p.s_start -= lo[k];
      p.s_end -= lo[k];
      res.rec[items[k]] = p;  // ops_offset: still within the chunk pair's words
      res.src[items[k]] = src[k];
    }
  });
  JoinWords(words, &res.rec, &res.ops);
  if (frame) {
    // every path's shifts
    for (size_t h = 0; h < hits.size(); ++h)
      for (uint32_t r = 0; r < res.rec[h].n_runs; ++r) {
        const uint32_t word = res.ops[res.rec[h].ops_offset + r];
        if ((word & 15u) >= 4) frame_info_[h].shifts += word >> 4;
      }
    AddStats(frame_stats_, StatsDelta(dev.times().frame, before.frame));
  } else {
    AddStats(band_stats_, StatsDelta(dev.times().band, before.band));
  }
  res.valid = true;
  return res;
}

const std::vector<GhostmHitFrameInfo> &Session::FrameInfo() {
  ReadLevel(true);
  return frame_info_;
}

// The read-level rows of every final hit (HitsReadRows): HitsRows' plan with
// the read-level paths. The hits' column counts give every hit its place in hit
// order, then one ReadRows call per (query chunk, DB chunk) writes the bytes
// there, with the source the path pass aligned and the subject coordinates made
// absolute in the chunk again.
const std::vector<GhostmHitReadRows> &Session::HitsReadRows(bool frame) {
  ReadRowsResult &res = read_rows_[frame ? 1 : 0];
  if (res.valid) return res.rec;
  const ReadLevelResult &lvl = ReadLevel(frame);
  const std::vector<uint32_t> &words = lvl.ops;
  res.rec.assign(Hits().size(), GhostmHitReadRows{0, 0, 0, 0, 0, 0, 0, 0, 0});
  DeviceModule &dev = DeviceModule::Get();
  const DeviceTimes before = dev.times();
  std::vector<GhostmBandSource> src;
  std::vector<GhostmHitReadRows> out;
  RowsPlan(lvl.rec, words, &res.bytes, [&](size_t qi, size_t di, const std::vector<size_t> &items,
                                        const std::vector<GhostmHitPath> &rec, const std::vector<uint64_t> &dst) {
    src.clear();
    for (size_t h : items) src.push_back(lvl.src[h]);
    out.resize(items.size());
    const uint32_t W = queries_[qi].chunk.L, step = tile_step_ ? tile_step_ : W;
    dev.ReadRows(queries_[qi].dev, dbs_[di].dev, (uint32_t)items.size(), src.data(), rec.data(), words.data(),
                 words.size(), step, frame, opt_.open_gap, opt_.extend_gap, frame_shift_, queries_[qi].global_base,
                 out.data(), res.bytes.data(), res.bytes.size(), dst.data());
    for (size_t k = 0; k < items.size(); ++k) res.rec[items[k]] = out[k];
  });
  AddStats(read_rows_stats_, StatsDelta(dev.times().read_rows, before.read_rows));
  res.valid = true;
  return res.rec;
}

const std::vector<uint8_t> &Session::ReadRowBytes(bool frame) {
  HitsReadRows(frame);
  return read_rows_[frame ? 1 : 0].bytes;
}

// -y 14 / -y 15: the -y 12 / -y 13 line, then positives, qseq and sseq: from
// the hit's read-level rows where its read-level score is above 0 (the line
// then describes that path), from its tile rows otherwise (the -y 8 fields of
// the tile path the line describes).
void Session::FormatReadRows(bool frame) {
  const std::vector<GhostmHitReadRows> &read = HitsReadRows(frame);
  const std::vector<uint8_t> &read_bytes = read_rows_[frame ? 1 : 0].bytes;
  const std::vector<GhostmHitPath> &level = level_[frame ? 1 : 0].rec;
  const std::vector<GhostmHitRows> &tile = HitsRows();
  const std::vector<uint8_t> &tile_bytes = row_bytes_;
  const auto extra = [&](size_t first, size_t n) {
    size_t need = n * 16;
    for (size_t i = 0; i < n; ++i) need += 2 * (size_t)std::max(read[first + i].columns, tile[first + i].columns);
    return need;
  };
  RewriteLines("read rows output", 0, extra,
               [&](size_t hit, const std::string &in, size_t pos, size_t nl, const size_t *, std::string &out) {
    const bool lvl = level[hit].score > 0;
    const size_t n = lvl ? read[hit].columns : tile[hit].columns;
    const uint32_t positives = lvl ? read[hit].positives : tile[hit].positives;
    const char *q = reinterpret_cast<const char *>(lvl ? read_bytes.data() + read[hit].rows_offset
                                                       : tile_bytes.data() + tile[hit].rows_offset);
    char num[16], *end = PutU32(num, positives);
    out.append(in, pos, nl - pos);
    out.push_back('\t');
    out.append(num, (size_t)(end - num));
    out.push_back('\t');
    out.append(q, n);
    out.push_back('\t');
    out.append(q + 2 * n, n);
    out.push_back('\n');
  });
}

// Strand position p of a read of read_nt nucleotides as a forward-strand
// position, from 0: what -y 13 prints (plus 1) and what the cull compares.
static inline uint32_t ForwardNt(uint32_t strand, uint32_t read_nt, uint32_t p) {
  return strand ? read_nt - 1 - p : p;
}

// -y 13: FormatPathTabular's line from the hit's frame path (HitsFrame) in read
// nucleotide coordinates, then qframe and frameshifts. A hit of frame score 0
// prints its tile path in the same units, with the style-0 line's E-value and
// bit score.
void Session::FormatFrameTabular() {
  const ReadLevelResult &lvl = ReadLevel(true);
  const std::vector<GhostmHitPath> &frame_path = lvl.rec;
  const std::vector<GhostmHitPath> &tile_path = HitsPath();
  const LineFormat &w = Format();
  RewriteLines("frame tabular output", 8, [](size_t, size_t n) { return n * 80; },
               [&](size_t hit, const std::string &in, size_t pos, size_t, const size_t *tab, std::string &out) {
    const bool framed = frame_path[hit].score > 0;
    const GhostmHitPath &x = framed ? frame_path[hit] : tile_path[hit];
    const std::vector<uint32_t> &ops = framed ? lvl.ops : path_ops_;
    const GhostmHitFrameInfo &info = frame_info_[hit];
    uint32_t count[4] = {0, 0, 0, 0}, gap_runs = 0;
    for (uint32_t r = 0; r < x.n_runs; ++r) {
      const uint32_t word = ops[x.ops_offset + r], op = word & 15u;
      if (op >= 4) continue;  // a shift is no column
      count[op] += word >> 4;
      gap_runs += op >= 2;
    }
    const uint32_t length = count[0] + count[1] + count[2] + count[3];
    out.append(in, pos, tab[7] + 1 - pos);
    char num[200], *p = num;
    p = w.PutId(p, length, count[0]); *p++ = '\t';
    p = PutU32(p, length); *p++ = '\t';
    p = PutU32(p, count[1]); *p++ = '\t';
    p = PutU32(p, gap_runs); *p++ = '\t';
    // strand positions of the first and the last nucleotide
    uint32_t q0 = x.q_start, q1 = x.q_end;
    if (!framed) {
      const GhostmQueryTile &t = tile_table_[queries_[hit_source_[hit].qi].global_base + hit_source_[hit].query];
      q0 = 3 * (t.offset + x.q_start) + t.frame % 3;
      q1 = 3 * (t.offset + x.q_end) + t.frame % 3 + 2;
    }
    p = PutU32(p, ForwardNt(info.strand, info.read_nt, q0) + 1); *p++ = '\t';
    p = PutU32(p, ForwardNt(info.strand, info.read_nt, q1) + 1); *p++ = '\t';
    p = PutU32(p, x.s_start + 1); *p++ = '\t';
    p = PutU32(p, x.s_end + 1); *p++ = '\t';
    if (framed) {
      const uint32_t m = info.letters;
      const float scaled = (float)((uint64_t)m * (uint64_t)db_sum_u32_) * w.ev.p.K;
      p = w.PutEvalue(p, m, x.score, scaled); *p++ = '\t';
      p = w.PutBits(p, x.score);
      out.append(num, (size_t)(p - num));
    } else {
      out.append(num, (size_t)(p - num));
      out.append(in, tab[2] + 1, tab[0] - tab[2] - 1);
    }
    out.push_back('\t');
    for (uint32_t r = 0; r < x.n_runs; ++r) {
      const uint32_t word = ops[x.ops_offset + r];
      p = PutU32(num, word >> 4);
      *p++ = "=XID\\/"[word & 7u];
      out.append(num, (size_t)(p - num));
    }
    p = num;
    *p++ = '\t';
    if (info.strand) *p++ = '-';
    p = PutU32(p, q0 % 3 + 1); *p++ = '\t';
    p = PutU32(p, framed ? info.shifts : 0u);
    *p++ = '\n';
    out.append(num, (size_t)(p - num));
  });
}

void Session::SetCull(uint32_t top_k, uint32_t cover_pct) {
  if (top_k < 1 || top_k > 255) throw Error("cull: param: top_k " + std::to_string(top_k) + " outside 1..255");
  if (cover_pct < 1 || cover_pct > 100)
    throw Error("cull: param: cover_pct " + std::to_string(cover_pct) + " outside 1..100");
  if (top_k == cull_top_k_ && cover_pct == cull_cover_pct_) return;
  cull_top_k_ = top_k;
  cull_cover_pct_ = cover_pct;
  DropLevel(0, kFromCull);
  DropLevel(1, kFromCull);
}

void Session::SetTileGroups(bool on) {
  if (shard_world_ > 1) throw Error("a shard session's query set cannot be replaced");
  tile_groups_ = on;
}

void Session::SetMask(uint32_t window, uint32_t trigger, uint32_t extend) {
  if (shard_world_ > 1) throw Error("a shard session's query set cannot be replaced");
  if (window == 0) {
    mask_ = MaskParams();
    return;
  }
  const std::string why = ValidateMaskParams(window, trigger, extend);
  if (!why.empty()) throw Error("mask: " + why);
  mask_.window = window;
  mask_.trigger = trigger;
  mask_.extend = extend;
}

void Session::SetQuality(uint32_t trim_q, uint32_t mask_q, uint32_t min_len) {
  if (shard_world_ > 1) throw Error("a shard session's query set cannot be replaced");
  const std::string why = ValidateQualParams(trim_q, mask_q, min_len);
  if (!why.empty()) throw Error("quality: " + why);
  qual_.trim_q = trim_q;
  qual_.mask_q = mask_q;
  qual_.min_len = min_len;
}

void Session::SetAdapters(const std::string &adapter1, const std::string &adapter2, uint32_t min_overlap,
                          uint32_t err_pct, uint32_t pair_overlap) {
  if (shard_world_ > 1) throw Error("a shard session's query set cannot be replaced");
  const std::string why =
      MakeAdapterParams(adapter1.c_str(), adapter2.c_str(), min_overlap, err_pct, pair_overlap, &adapter_);  // sets it only on ""
  if (!why.empty()) throw Error("adapters: " + why);
}

double Session::MaskChunk(QueryData *q, const std::vector<GhostmBandSource> &src, uint32_t step) {
  q->masked.assign(q->chunk.nseq, 0);
  GhostmMaskStats one{};
  DeviceModule::Get().MaskQuery(q->dev, (uint32_t)src.size(), src.data(), step, mask_, q->masked.data(), &one);
  mask_stats_.seconds_mask += one.seconds_mask;
  mask_stats_.mask_launches += one.mask_launches;
  mask_stats_.mask_sources += one.mask_sources;
  mask_stats_.mask_windows += one.mask_windows;
  mask_stats_.masked_sources += one.masked_sources;
  mask_stats_.masked_letters += one.masked_letters;
  return one.seconds_mask;
}

std::vector<uint32_t> Session::AllQueryMasked() const {
  std::vector<uint32_t> out;
  for (const QueryData &q : queries_) out.insert(out.end(), q.masked.begin(), q.masked.end());
  return out;
}

// The cull's input record of final hit h (ReadCull; ReadLca for the hits the
// cull kept). The reads: consecutive hits of one
// source record (tiled set) or of one name group (untiled set). A hit's record
// is its read-level path's: the q interval in forward-strand read units
// (nucleotides on a tiled DNA set: a band path's frame letters c of frame f
// cover strand positions 3c + f % 3 to 3c + f % 3 + 2, a frame path's q_* are
// strand positions already; ForwardNt turns the reverse strand's round).
GhostmCullHit Session::CullRecord(bool frame, size_t h, const GhostmHit &hit, const GhostmHitPath &x, uint64_t *key) const {
  const HitSource &hs = hit_source_[h];
  const QueryData &q = queries_[hs.qi];
  const bool tiled = !tile_table_.empty();
  const GhostmQueryTile *t = tiled ? &tile_table_[q.global_base + hs.query] : nullptr;
  // the read's key: the source record, or the name group's end over all chunks
  if (key) *key = tiled ? t->record : (uint64_t)q.global_base + q.group_end[hs.query];
  GhostmCullHit c{hit.db_id, x.score, 0, 0, x.s_start, x.s_end};
  if (x.score) {
    if (tiled && tile_dna_) {
      const uint32_t g = t->frame % 3, strand = t->frame / 3, nt = tile_read_nt_[t->record];
      const uint32_t p0 = frame ? x.q_start : 3 * x.q_start + g, p1 = frame ? x.q_end : 3 * x.q_end + g + 2;
      const uint32_t a = ForwardNt(strand, nt, p0), b = ForwardNt(strand, nt, p1);
      c.q_lo = std::min(a, b);
      c.q_hi = std::max(a, b);
    } else {
      c.q_lo = x.q_start;
      c.q_hi = x.q_end;
    }
  } else {
    c.s_lo = c.s_hi = 0;  // an EMPTY hit: its ranges say nothing
  }
  return c;
}

const Session::ReadCullResult &Session::ReadCull(bool frame) {
  ReadCullResult &res = cull_[frame ? 1 : 0];
  if (res.valid) return res;
  const std::vector<GhostmHitPath> &path = ReadLevel(frame).rec;
  const std::vector<GhostmHit> &hits = Hits();
  const size_t n = hits.size();
  if (n > UINT32_MAX) throw Error("read cull: over 4 G hits");
  std::vector<GhostmCullHit> in(n);
  res.read_begin.assign(1, 0);
  uint64_t prev = UINT64_MAX;
  for (size_t h = 0; h < n; ++h) {
    uint64_t key = 0;
    in[h] = CullRecord(frame, h, hits[h], path[h], &key);
    if (h && key != prev) res.read_begin.push_back((uint32_t)h);
    prev = key;
  }
  res.read_begin.push_back((uint32_t)n);
  res.out.assign(n, GhostmCullOut{0, GHOSTM_CULL_EMPTY, 0xFFFFFFFFu, 0});
  DeviceModule &dev = DeviceModule::Get();
  const DeviceTimes before = dev.times();
  dev.ReadCull((uint32_t)res.read_begin.size() - 1, res.read_begin.data(), (uint32_t)n, in.data(), cull_top_k_,
               cull_cover_pct_, res.out.data());
  AddStats(cull_stats_, StatsDelta(dev.times().cull, before.cull));
  res.valid = true;
  return res;
}

// -y 20 / -y 21: the -y 12 / -y 13 lines are in the parts, one per hit in hit
// order. A read's hits may lie in several parts (tile groups), so the lines are
// found over all the parts' text and the new text is assembled per read: the
// KEPT hits in kept_rank order, each line with its rank and its covered count.
void Session::FormatCull(bool frame) {
  const ReadCullResult &res = ReadCull(frame);
  struct LineAt {
    const std::string *text;
    size_t pos, len;  // without the newline
  };
  std::vector<LineAt> line;
  line.reserve(res.out.size());
  size_t bytes = 0;
  for (size_t k = 0; k < used_parts_; ++k)
    for (size_t t = 0; t < parts_[k].text.size(); ++t) {
      const std::string &in = parts_[k].text[t];
      size_t pos = 0;
      for (size_t i = 0; i < parts_[k].hits[t].size(); ++i) {
        const size_t nl = in.find('\n', pos);
        if (nl == std::string::npos) throw Error("cull output: fewer lines than hits");
        line.push_back(LineAt{&in, pos, nl - pos});
        pos = nl + 1;
      }
      bytes += in.size();
    }
  if (line.size() != res.out.size()) throw Error("cull output: the lines are not the hits'");
  std::string out;
  out.reserve(bytes);
  std::vector<uint32_t> by_rank;
  for (size_t r = 0; r + 1 < res.read_begin.size(); ++r) {
    const uint32_t b = res.read_begin[r], e = res.read_begin[r + 1];
    by_rank.clear();
    for (uint32_t h = b; h < e; ++h)
      if (res.out[h].status == GHOSTM_CULL_KEPT) by_rank.push_back(h);
    std::sort(by_rank.begin(), by_rank.end(),
              [&](uint32_t x, uint32_t y) { return res.out[x].kept_rank < res.out[y].kept_rank; });
    for (uint32_t h : by_rank) {
      out.append(*line[h].text, line[h].pos, line[h].len);
      char num[32], *p = num;
      *p++ = '\t';
      p = PutU32(p, res.out[h].kept_rank); *p++ = '\t';
      p = PutU32(p, res.out[h].detail); *p++ = '\n';
      out.append(num, (size_t)(p - num));
    }
  }
  ReplaceText(&out);
}

// The text of a view that is not one line per hit (the culled lines, the taxon
// lines, the pile-up lines) replaces the hit lines: it goes into the first
// part's first piece, every other piece is emptied.
void Session::ReplaceText(std::string *out) {
  bool placed = false;
  for (size_t k = 0; k < used_parts_; ++k)
    for (std::string &t : parts_[k].text) {
      t.clear();
      if (!placed) t.swap(*out), placed = true;
    }
  joined_valid_ = false;
}

static std::string ReadTextFile(const std::string &path, const char *what) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f) throw Error(std::string("set taxonomy: cannot open the ") + what + " file " + path);
  std::ostringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

void Session::SetTaxonomy(uint32_t nnodes, const uint32_t *taxid, const uint32_t *parent, size_t nsubjects,
                          const uint32_t *subject_node, uint64_t map_unmatched) {
  if (!taxid || !parent) throw Error("set taxonomy: null: taxid or parent");
  if (nsubjects && !subject_node) throw Error("set taxonomy: null: subject_node");
  std::vector<uint32_t> depth;
  const std::string why = TaxonomyDepths(nnodes, parent, &depth);
  if (!why.empty()) throw Error("set taxonomy: " + why);
  std::unordered_set<uint32_t> seen;
  for (uint32_t i = 0; i < nnodes; ++i) {
    if (taxid[i] == 0) throw Error("set taxonomy: taxonomy: node " + std::to_string(i) + ": taxid 0");
    if (!seen.insert(taxid[i]).second)
      throw Error("set taxonomy: taxonomy: node " + std::to_string(i) + ": taxid " + std::to_string(taxid[i]) + " repeated");
  }
  const size_t have = dbs_.empty() ? 0 : (size_t)dbs_.back().global_base + dbs_.back().chunk.nseq;
  if (nsubjects != have)
    throw Error("set taxonomy: subjects: " + std::to_string(nsubjects) + " given, the database has " + std::to_string(have));
  uint64_t mapped = 0;
  for (size_t k = 0; k < nsubjects; ++k) {
    if (subject_node[k] != kLcaNone && subject_node[k] >= nnodes)
      throw Error("set taxonomy: node: subject " + std::to_string(k) + ": no such node");
    mapped += subject_node[k] != kLcaNone;
  }
  DeviceModule &dev = DeviceModule::Get();
  dev.SetTaxonomy(nnodes, parent);
  tax_.taxid.assign(taxid, taxid + nnodes);
  tax_.parent.assign(parent, parent + nnodes);
  tax_.subject_node.assign(subject_node, subject_node + nsubjects);
  tax_.mapped = mapped;
  tax_.map_unmatched = map_unmatched;
  tax_.serial = dev.taxonomy_serial();
  tax_.depth = depth;
  tax_.set = true;
  DropLevel(0, kFromLca);
  DropLevel(1, kFromLca);
}

void Session::SetTaxonomyFiles(const std::string &nodes_path, const std::string &map_path) {
  TaxonomyFile nodes;
  std::string why = ParseTaxonomyNodes(ReadTextFile(nodes_path, "nodes"), &nodes);
  if (!why.empty()) throw Error("set taxonomy: " + why);
  std::vector<std::pair<std::string, uint32_t>> lines;
  std::vector<uint32_t> line_of;
  why = ParseTaxonomyMap(ReadTextFile(map_path, "map"), &lines, &line_of);
  if (!why.empty()) throw Error("set taxonomy: " + why);
  std::unordered_map<uint32_t, uint32_t> node_of;
  for (size_t i = 0; i < nodes.taxid.size(); ++i) node_of.emplace(nodes.taxid[i], (uint32_t)i);
  std::unordered_map<std::string, uint32_t> name_node;  // a later line wins
  for (size_t k = 0; k < lines.size(); ++k) {
    const auto it = node_of.find(lines[k].second);
    if (it == node_of.end())
      throw Error("set taxonomy: map: line " + std::to_string(line_of[k]) + ": taxid " + std::to_string(lines[k].second) +
                  " is not in the nodes file");
    name_node[lines[k].first] = it->second;
  }
  std::vector<uint32_t> subject_node;
  std::unordered_set<std::string> names;
  for (const DbData &d : dbs_)
    for (uint32_t s = 0; s < d.chunk.nseq; ++s) {
      const std::string key = LcaNameKey(std::string(d.chunk.names[s]));
      const auto it = name_node.find(key);
      subject_node.push_back(it == name_node.end() ? kLcaNone : it->second);
      names.insert(key);
    }
  uint64_t unmatched = 0;
  for (const auto &l : lines) unmatched += names.count(l.first) == 0;
  SetTaxonomy((uint32_t)std::min<size_t>(nodes.taxid.size(), UINT32_MAX), nodes.taxid.data(), nodes.parent.data(),
              subject_node.size(), subject_node.data(), unmatched);
}

GhostmTaxonomyInfo Session::TaxonomyInfo() const {
  GhostmTaxonomyInfo info{};
  if (!tax_.set) return info;
  info.nodes = tax_.taxid.size();
  info.subjects_mapped = tax_.mapped;
  info.subjects_unmapped = tax_.subject_node.size() - tax_.mapped;
  info.map_unmatched = tax_.map_unmatched;
  return info;
}

void Session::SetLca(uint32_t top_pct, uint32_t support_pct) {
  if (top_pct > 100) throw Error("lca: param: top_pct " + std::to_string(top_pct) + " outside 0..100");
  if (support_pct < 51 || support_pct > 100)
    throw Error("lca: param: support_pct " + std::to_string(support_pct) + " outside 51..100");
  if (top_pct == lca_top_pct_ && support_pct == lca_support_pct_) return;
  lca_top_pct_ = top_pct;
  lca_support_pct_ = support_pct;
  DropLevel(0, kFromLca);
  DropLevel(1, kFromLca);
}

// The taxon of every read (ReadLca): the cull's reads and records, a KEPT hit
// a candidate with its read-level score, every other hit score 0.
const Session::ReadLcaResult &Session::ReadLca(bool frame) {
  if (!tax_.set) throw Error("read lca: taxonomy: none is set (GhostmSessionSetTaxonomy)");
  ReadLcaResult &res = lca_[frame ? 1 : 0];
  if (res.valid) return res;
  const ReadCullResult &cull = ReadCull(frame);
  const std::vector<GhostmHitPath> &path = ReadLevel(frame).rec;
  const std::vector<GhostmHit> &hits = Hits();
  const size_t n = hits.size();
  res.read_begin = cull.read_begin;
  if (n == 0) res.read_begin.assign(1, 0);  // no hit, no read
  // Only the KEPT hits go to the stage call: every other hit has score 0 there,
  // is no candidate and changes no field of the record. begin: the reads in
  // the compacted array.
  std::vector<GhostmLcaHit> rec;
  std::vector<uint32_t> begin(res.read_begin.size());
  for (size_t r = 0; r + 1 < res.read_begin.size(); ++r) {
    begin[r] = (uint32_t)rec.size();
    for (uint32_t h = res.read_begin[r]; h < res.read_begin[r + 1]; ++h) {
      if (cull.out[h].status != GHOSTM_CULL_KEPT) continue;
      const GhostmCullHit c = CullRecord(frame, h, hits[h], path[h], nullptr);
      rec.push_back(GhostmLcaHit{tax_.subject_node[hits[h].db_id], c.score, c.q_lo, c.q_hi});
    }
  }
  begin.back() = (uint32_t)rec.size();
  DeviceModule &dev = DeviceModule::Get();
  if (dev.taxonomy_serial() != tax_.serial) {  // SetTaxonomyGpu, FreeGpu or another session since: ours again
    dev.SetTaxonomy((uint32_t)tax_.parent.size(), tax_.parent.data());
    tax_.serial = dev.taxonomy_serial();
  }
  const uint32_t nreads = (uint32_t)res.read_begin.size() - 1;
  res.out.assign(nreads, GhostmLcaOut{});
  const GhostmReadLcaStats before = dev.times().lca;
  dev.ReadLca(nreads, begin.data(), (uint32_t)rec.size(), rec.data(), lca_top_pct_, lca_support_pct_, res.out.data());
  GhostmReadLcaStats added = StatsDelta(dev.times().lca, before);
  added.lca_reads = nreads;  // the session's reads and hits, not the compacted call's
  added.lca_hits = n;
  AddStats(lca_stats_, added);
  res.valid = true;
  return res;
}

// -y 22 / -y 23: one line per read, named by its first hit's query record.
void Session::FormatLca(bool frame) {
  const ReadLcaResult &res = ReadLca(frame);
  std::string out;
  for (size_t r = 0; r + 1 < res.read_begin.size(); ++r) {
    const HitSource &hs = hit_source_[res.read_begin[r]];
    const GhostmLcaOut &o = res.out[r];
    out.append(queries_[hs.qi].chunk.names[hs.query]);
    const uint32_t cols[8] = {o.node == kLcaNone ? 0u : tax_.taxid[o.node], o.depth, o.votes, o.support,
                              o.lca == kLcaNone ? 0u : tax_.taxid[o.lca], o.candidates, o.unmapped, o.best_score};
    for (uint32_t c : cols) {
      char num[16], *p = num;
      *p++ = '\t';
      p = PutU32(p, c);
      out.append(num, (size_t)(p - num));
    }
    out.push_back('\n');
  }
  ReplaceText(&out);
}

void Session::SetMates(bool on, uint32_t max_insert) {
  if (shard_world_ > 1) throw Error("a shard session has no mates");
  if (max_insert < 1 || max_insert > kPairValueLimit)
    throw Error("mates: param: max_insert " + std::to_string(max_insert) + " outside 1..2^24");
  if (on == mates_ && max_insert == mates_max_insert_) return;
  mates_ = on;
  mates_max_insert_ = max_insert;
  for (int lv = 0; lv < 2; ++lv) {  // the pair results and what is counted from them; the cull and the per-read taxa stay
    pair_[lv].Drop();
    pair_lca_[lv].Drop();
    profile_[lv].Drop();
  }
}

// Why a pair pass cannot run, or "".
std::string Session::MatesRefusal() const {
  if (!mates_) return "mates: they are off (GhostmSessionSetMates)";
  if (tile_table_.empty()) return "mates: the query set is not tiled";
  if (tile_read_nt_.size() % 2) return "mates: " + std::to_string(tile_read_nt_.size()) + " source records, an odd number";
  return std::string();
}

// The join of every pair's hits (PairJoin): source records 2p and 2p + 1 are
// the mates of pair p. The cull's reads in order, a KEPT hit a candidate with
// the cull's record, its subject's node and its tile's strand, every other hit
// score 0. A pair is there when either mate has a hit.
const Session::PairJoinResult &Session::PairJoin(bool frame) {
  const std::string why = MatesRefusal();
  if (!why.empty()) throw Error("pair join: " + why);
  PairJoinResult &res = pair_[frame ? 1 : 0];
  if (res.valid) return res;
  const ReadCullResult &cull = ReadCull(frame);
  const std::vector<GhostmHitPath> &path = ReadLevel(frame).rec;
  const std::vector<GhostmHit> &hits = Hits();
  const size_t n = hits.size();
  std::vector<GhostmPairHit> in(n, GhostmPairHit{0, kPairNone, 0, 0, 0, 0, 0, 0});
  res.pair_begin.assign(1, 0);
  res.pair_record.clear();
  std::vector<uint32_t> offset;
  uint64_t prev_pair = UINT64_MAX;
  for (size_t r = 0; r + 1 < cull.read_begin.size() && n; ++r) {
    const uint32_t b = cull.read_begin[r], e = cull.read_begin[r + 1];
    uint64_t record = 0;
    for (uint32_t h = b; h < e; ++h) {
      const GhostmCullHit c = CullRecord(frame, h, hits[h], path[h], &record);
      if (cull.out[h].status != GHOSTM_CULL_KEPT) continue;
      const HitSource &hs = hit_source_[h];
      const GhostmQueryTile &t = tile_table_[queries_[hs.qi].global_base + hs.query];
      in[h] = GhostmPairHit{c.subject, tax_.set ? tax_.subject_node[hits[h].db_id] : kPairNone, c.score, c.q_lo, c.q_hi,
                            c.s_lo, c.s_hi, tile_dna_ ? t.frame / 3 : 0u};
    }
    const uint64_t pair = record >> 1;
    if (pair != prev_pair) {
      if (prev_pair != UINT64_MAX && pair < prev_pair) throw Error("pair join: internal: the reads are not in record order");
      if (prev_pair != UINT64_MAX) {  // close the pair before: without a mate 2 it ends where that would begin
        if (res.pair_begin.size() % 2 == 1) res.pair_begin.push_back(b);
        res.pair_begin.push_back(b);
      }
      prev_pair = pair;
      res.pair_record.push_back((uint32_t)(2 * pair));
      offset.push_back(tile_read_nt_[2 * pair]);
      if (record & 1) res.pair_begin.push_back(b);  // mate 1 has no hit
    } else {
      res.pair_begin.push_back(b);  // mate 2 begins
    }
  }
  if (prev_pair != UINT64_MAX) {
    if (res.pair_begin.size() % 2 == 1) res.pair_begin.push_back((uint32_t)n);
    res.pair_begin.push_back((uint32_t)n);
  }
  const uint32_t npairs = (uint32_t)res.pair_record.size();
  if (res.pair_begin.size() != 2 * (size_t)npairs + 1) throw Error("pair join: internal: the pairs' borders");
  res.cand.assign(n, GhostmLcaHit{0, 0, 0, 0});
  res.partner.assign(n, kPairNone);
  res.out.assign(npairs, GhostmPairOut{0, 0, 0, 0});
  const uint32_t max_span = tile_dna_ ? std::max(1u, mates_max_insert_ / 3) : mates_max_insert_;
  DeviceModule &dev = DeviceModule::Get();
  const GhostmPairJoinStats before = dev.times().pair;
  dev.PairJoin(npairs, res.pair_begin.data(), offset.data(), (uint32_t)n, in.data(), max_span, tile_dna_ ? 1u : 0u,
               res.cand.data(), res.partner.data(), res.out.data());
  AddStats(pair_stats_, StatsDelta(dev.times().pair, before));
  res.valid = true;
  return res;
}

// The taxon of every pair (PairLca): one ReadLca call over the joined
// candidates with the pairs as reads.
const Session::PairLcaResult &Session::PairLca(bool frame) {
  if (!tax_.set) throw Error("pair lca: taxonomy: none is set (GhostmSessionSetTaxonomy)");
  const PairJoinResult &join = PairJoin(frame);
  PairLcaResult &res = pair_lca_[frame ? 1 : 0];
  if (res.valid) return res;
  const uint32_t npairs = (uint32_t)join.out.size();
  std::vector<uint32_t> begin(npairs + (size_t)1);
  for (uint32_t p = 0; p <= npairs; ++p) begin[p] = join.pair_begin[2 * (size_t)p];
  DeviceModule &dev = DeviceModule::Get();
  if (dev.taxonomy_serial() != tax_.serial) {  // SetTaxonomyGpu, FreeGpu or another session since: ours again
    dev.SetTaxonomy((uint32_t)tax_.parent.size(), tax_.parent.data());
    tax_.serial = dev.taxonomy_serial();
  }
  res.out.assign(npairs, GhostmLcaOut{});
  const GhostmReadLcaStats before = dev.times().lca;
  dev.ReadLca(npairs, begin.data(), (uint32_t)join.cand.size(), join.cand.data(), lca_top_pct_, lca_support_pct_,
              res.out.data());
  AddStats(lca_stats_, StatsDelta(dev.times().lca, before));
  res.valid = true;
  return res;
}

// The name of source record `record` of a tiled set: its first tile record's.
std::string Session::SourceName(uint32_t record) const {
  const auto it = std::lower_bound(tile_table_.begin(), tile_table_.end(), record,
                                   [](const GhostmQueryTile &t, uint32_t r) { return t.record < r; });
  const uint32_t g = (uint32_t)(it - tile_table_.begin());
  for (const QueryData &q : queries_)
    if (g >= q.global_base && g - q.global_base < q.chunk.nseq) return std::string(q.chunk.names[g - q.global_base]);
  throw Error("pair output: internal: no tile record of source record " + std::to_string(record));
}

// -y 26 / -y 27: one line per pair with a hit, named by mate 1's record.
void Session::FormatPairLca(bool frame) {
  const PairLcaResult &res = PairLca(frame);
  const PairJoinResult &join = PairJoin(frame);
  std::string out;
  for (size_t p = 0; p < res.out.size(); ++p) {
    const GhostmLcaOut &o = res.out[p];
    const GhostmPairOut &j = join.out[p];
    out.append(SourceName(join.pair_record[p]));
    const uint32_t cols[11] = {o.node == kLcaNone ? 0u : tax_.taxid[o.node], o.depth, o.votes, o.support,
                               o.lca == kLcaNone ? 0u : tax_.taxid[o.lca], o.candidates, o.unmapped, o.best_score,
                               j.mates, j.joined, j.best_span};
    for (uint32_t c : cols) {
      char num[16], *p2 = num;
      *p2++ = '\t';
      p2 = PutU32(p2, c);
      out.append(num, (size_t)(p2 - num));
    }
    out.push_back('\n');
  }
  ReplaceText(&out);
}

void Session::SetProfile(uint32_t min_reads) {
  if (min_reads < 1) throw Error("profile: param: min_reads 0");
  if (min_reads == profile_min_reads_) return;
  profile_min_reads_ = min_reads;
  profile_[0].Drop();  // the assignments under them stay
  profile_[1].Drop();
}

// The sample's profile (TaxonProfile): every ReadLca record is a read, its node the read's. With mates on every
// PairLca record is a fragment, counted once.
const Session::TaxonProfileResult &Session::TaxonProfile(bool frame) {
  const std::vector<GhostmLcaOut> &lca = mates_ ? PairLca(frame).out : ReadLca(frame).out;  // throws without a taxonomy
  TaxonProfileResult &res = profile_[frame ? 1 : 0];
  if (res.valid) return res;
  const uint32_t nreads = (uint32_t)lca.size();
  std::vector<uint32_t> node(nreads);
  for (uint32_t r = 0; r < nreads; ++r) node[r] = lca[r].node;
  DeviceModule &dev = DeviceModule::Get();
  if (dev.taxonomy_serial() != tax_.serial) {  // SetTaxonomyGpu, FreeGpu or another session since: ours again
    dev.SetTaxonomy((uint32_t)tax_.parent.size(), tax_.parent.data());
    tax_.serial = dev.taxonomy_serial();
  }
  const GhostmTaxonProfileStats before = dev.times().profile;
  size_t n = 0;
  res.final_node.assign(nreads, kLcaNone);
  res.summary = GhostmTaxonSummary{};
  dev.TaxonProfile(nreads, node.data(), profile_min_reads_, 0, nullptr, &n, res.final_node.data(), &res.summary, &res.rec);
  AddStats(profile_stats_, StatsDelta(dev.times().profile, before));
  res.valid = true;
  return res;
}

// -y 24 / -y 25: the report of the whole sample.
void Session::FormatProfile(bool frame) {
  const TaxonProfileResult &res = TaxonProfile(frame);
  std::string out = TaxonReport(res.rec.data(), res.rec.size(), profile_min_reads_, res.summary.reads, tax_.parent.data(),
                                tax_.depth.data(), tax_.taxid.data());
  ReplaceText(&out);
}

// A subject's residues: every subject of a chunk is followed by one END.
uint32_t Session::SubjectLength(const DbData &d, uint32_t subject) const {
  const uint32_t next = subject + 1 < d.chunk.nseq ? d.chunk.starts[subject + 1] : d.chunk.len;
  return next - d.chunk.starts[subject] - 1;
}

const std::vector<GhostmHitPath> &Session::LevelPaths(PathLevel lv) {
  return lv == kTileLevel ? HitsPath() : ReadLevel(lv == kFrameLevel).rec;
}

// One pile-up call on DB chunk di for the hits `items`: the hits by query chunk
// with their subject coordinates absolute in the chunk again, the tile paths'
// resolved records (PathPileup) or the sources HitsBand() / HitsFrame() aligned
// (ReadPileup).
void Session::PileupChunk(PathLevel lv, size_t di, const std::vector<size_t> &items, uint32_t p0, uint32_t p1,
                          uint32_t *depth, uint32_t *identities, uint8_t *consensus, uint32_t *shifts,
                          uint32_t *profile) {
  const bool tile = lv == kTileLevel, frame = lv == kFrameLevel;
  const std::vector<GhostmHitPath> &path = LevelPaths(lv);
  const ReadLevelResult &lvl = level_[frame ? 1 : 0];  // made by LevelPaths; unused on the tile level
  const std::vector<uint32_t> &words = tile ? path_ops_ : lvl.ops;
  const std::vector<GhostmHit> &hits = Hits();
  std::vector<std::vector<uint32_t>> qid(queries_.size());
  std::vector<std::vector<GhostmBandSource>> src(queries_.size());
  std::vector<std::vector<GhostmHitPath>> rec(queries_.size());
  for (size_t h : items) {
    GhostmHitPath p = path[h];
    const uint32_t pos = dbs_[di].chunk.starts[hits[h].db_id - dbs_[di].global_base];
    p.s_start += pos;
    p.s_end += pos;
    if (tile) qid[hit_source_[h].qi].push_back(hit_source_[h].query);
    else src[hit_source_[h].qi].push_back(lvl.src[h]);
    rec[hit_source_[h].qi].push_back(p);
  }
  std::vector<DeviceModule::PileupGroup> tile_groups;
  std::vector<DeviceModule::ReadPileupGroup> groups;
  uint32_t step = 0;
  for (size_t qi = 0; qi < queries_.size(); ++qi) {
    if (rec[qi].empty()) continue;
    const uint32_t n = (uint32_t)rec[qi].size();
    if (tile) tile_groups.push_back(DeviceModule::PileupGroup{queries_[qi].dev, n, qid[qi].data(), rec[qi].data()});
    else groups.push_back(DeviceModule::ReadPileupGroup{queries_[qi].dev, n, src[qi].data(), rec[qi].data()});
    step = tile_step_ ? tile_step_ : queries_[qi].chunk.L;  // every chunk of a set has the same width
  }
  DeviceModule &dev = DeviceModule::Get();
  const DeviceTimes before = dev.times();
  if (tile) {
    dev.PathPileup(dbs_[di].dev, tile_groups.data(), tile_groups.size(), words.data(), words.size(), p0, p1, depth,
                   identities, consensus, profile);
    AddDeltas(stats_, before, dev.times(), std::make_pair(&GhostmStats::seconds_pileup, &DeviceTimes::pileup),
              std::make_pair(&GhostmStats::pileup_launches, &DeviceTimes::pileup_launches),
              std::make_pair(&GhostmStats::pileup_windows, &DeviceTimes::pileup_windows),
              std::make_pair(&GhostmStats::pileup_parts, &DeviceTimes::pileup_parts),
              std::make_pair(&GhostmStats::pileup_columns, &DeviceTimes::pileup_columns));
    return;
  }
  dev.ReadPileup(dbs_[di].dev, groups.data(), groups.size(), words.data(), words.size(), step, frame, p0, p1, depth,
                 identities, consensus, shifts, profile);
  AddStats(read_pileup_stats_, StatsDelta(dev.times().read_pileup, before.read_pileup));
}

// The pile-up of one level's paths: every subject placed in db_id order, one
// PileupChunk per DB chunk with hits, the subjects' arrays copied out and
// summed. The tile pile-up has no shifts.
const Session::ReadPileupResult &Session::PileupAt(PathLevel lv) {
  ReadPileupResult &res = pileup_[lv];
  if (res.valid) return res;
  LevelPaths(lv);  // the frame paths refuse what GhostmSessionHitsFrame refuses, before anything is made
  const bool with_shifts = lv != kTileLevel;
  const std::vector<GhostmHit> &hits = Hits();
  size_t nsubj = 0;
  uint64_t total = 0;
  for (const DbData &d : dbs_) {
    nsubj = std::max<size_t>(nsubj, (size_t)d.global_base + d.chunk.nseq);
    total += d.chunk.len - d.chunk.nseq;
  }
  res.subj.assign(nsubj, GhostmSubjectReadPileup{0, 0, 0, 0, 0, 0, 0, 0});
  res.depth.assign(total, 0);
  res.ident.assign(total, 0);
  res.shifts.assign(with_shifts ? total : 0, 0);
  res.cons.assign(total, 255);
  // every subject's place: db_id order is chunk order, subject order within a chunk
  std::vector<size_t> order(dbs_.size());
  for (size_t di = 0; di < dbs_.size(); ++di) order[di] = di;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return dbs_[a].global_base < dbs_[b].global_base; });
  uint64_t at = 0;
  for (size_t di : order)
    for (uint32_t s = 0; s < dbs_[di].chunk.nseq; ++s) {
      GhostmSubjectReadPileup &x = res.subj[dbs_[di].global_base + s];
      x.length = SubjectLength(dbs_[di], s);
      x.offset = at;
      at += x.length;
    }
  std::vector<std::vector<size_t>> by_db(dbs_.size());
  for (size_t h = 0; h < hits.size(); ++h) {
    by_db[hit_source_[h].di].push_back(h);
    ++res.subj[hits[h].db_id].hits;
  }
  std::vector<uint32_t> depth, ident, shifts;
  std::vector<uint8_t> cons;
  for (size_t di = 0; di < dbs_.size(); ++di) {
    if (by_db[di].empty()) continue;  // nothing landed on the chunk: zeros and 255s
    const DbData &d = dbs_[di];
    depth.assign(d.chunk.len, 0);
    ident.assign(d.chunk.len, 0);
    shifts.assign(with_shifts ? d.chunk.len : 0, 0);
    cons.assign(d.chunk.len, 255);
    PileupChunk(lv, di, by_db[di], 0, d.chunk.len, depth.data(), ident.data(), cons.data(),
                with_shifts ? shifts.data() : nullptr, nullptr);
    for (uint32_t s = 0; s < d.chunk.nseq; ++s) {
      GhostmSubjectReadPileup &x = res.subj[d.global_base + s];
      if (!x.hits || !x.length) continue;
      const uint32_t p = d.chunk.starts[s];
      std::copy(depth.begin() + p, depth.begin() + p + x.length, res.depth.begin() + x.offset);
      std::copy(ident.begin() + p, ident.begin() + p + x.length, res.ident.begin() + x.offset);
      if (with_shifts) std::copy(shifts.begin() + p, shifts.begin() + p + x.length, res.shifts.begin() + x.offset);
      std::copy(cons.begin() + p, cons.begin() + p + x.length, res.cons.begin() + x.offset);
      for (uint32_t k = 0; k < x.length; ++k) {
        const uint32_t v = depth[p + k];
        x.covered += v > 0;
        x.max_depth = std::max(x.max_depth, v);
        x.depth_sum += v;
        x.identities_sum += ident[p + k];
        if (with_shifts) x.shifts_sum += shifts[p + k];
      }
    }
  }
  // the tile pile-up's records as the C ABI hands them out: the first 40 bytes
  if (lv == kTileLevel) {
    pileup_subj_.clear();
    for (const GhostmSubjectReadPileup &x : res.subj)
      pileup_subj_.push_back(
          GhostmSubjectPileup{x.length, x.hits, x.covered, x.max_depth, x.depth_sum, x.identities_sum, x.offset});
  }
  res.valid = true;
  return res;
}

const std::vector<GhostmSubjectPileup> &Session::Pileup() {
  PileupAt(kTileLevel);
  return pileup_subj_;
}

const std::vector<uint32_t> &Session::PileupDepth() { return PileupAt(kTileLevel).depth; }
const std::vector<uint32_t> &Session::PileupIdentities() { return PileupAt(kTileLevel).ident; }
const std::vector<uint8_t> &Session::PileupConsensus() { return PileupAt(kTileLevel).cons; }

const Session::ReadPileupResult &Session::ReadPileup(bool frame) { return PileupAt(frame ? kFrameLevel : kBandLevel); }

// One subject's profile rows from one level's paths; what: the messages' prefix.
std::vector<uint32_t> Session::SubjectProfileAt(PathLevel lv, const char *what, uint32_t db_id, bool count_only) {
  if (!count_only) LevelPaths(lv);
  const std::vector<GhostmHit> &hits = Hits();
  size_t di = 0;
  while (di < dbs_.size() && !(db_id >= dbs_[di].global_base && db_id - dbs_[di].global_base < dbs_[di].chunk.nseq))
    ++di;
  if (di == dbs_.size()) throw Error(std::string(what) + ": db_id outside the loaded chunks");
  const uint32_t s = db_id - dbs_[di].global_base, len = SubjectLength(dbs_[di], s);
  std::vector<uint32_t> profile((size_t)len * 32, 0);
  std::vector<size_t> items;
  if (count_only) return profile;
  for (size_t h = 0; h < hits.size(); ++h)
    if (hits[h].db_id == db_id) items.push_back(h);
  if (len && !items.empty()) {
    const uint32_t p = dbs_[di].chunk.starts[s];
    PileupChunk(lv, di, items, p, p + len, nullptr, nullptr, nullptr, nullptr, profile.data());
  }
  return profile;
}

std::vector<uint32_t> Session::SubjectProfile(uint32_t db_id, bool count_only) {
  return SubjectProfileAt(kTileLevel, "subject profile", db_id, count_only);
}

std::vector<uint32_t> Session::ReadSubjectProfile(bool frame, uint32_t db_id, bool count_only) {
  return SubjectProfileAt(frame ? kFrameLevel : kBandLevel, "read subject profile", db_id, count_only);
}

// -y 10, -y 11 (the tile paths) and -y 16 to -y 19 (the read-level paths): one
// line per subject with at least one hit, in db_id order: name, length, hits,
// covered, depth_sum, identities_sum, max_depth, the frame pile-up's line (-y
// 18, -y 19) shifts_sum too, and last, with consensus, the consensus text (the
// residue letter, '-' where depth > 0 and no residue was seen, '.' where depth
// is 0). The text replaces the hit lines: it goes into the first piece, the
// other pieces are emptied.
void Session::FormatPileup(PathLevel lv, bool consensus) {
  const ReadPileupResult &res = PileupAt(lv);
  static const char kLetters[] = "ARNDCQEGHILKMFPSTWYVBJZX*";  // formats.cpp's order
  std::string out;
  for (const DbData &d : dbs_)
    for (uint32_t s = 0; s < d.chunk.nseq; ++s) {
      const GhostmSubjectReadPileup &x = res.subj[d.global_base + s];
      if (!x.hits) continue;
      out.append(d.chunk.names[s]);
      const uint64_t cols[7] = {x.length, x.hits, x.covered, x.depth_sum, x.identities_sum, x.max_depth, x.shifts_sum};
      for (size_t c = 0; c < (lv == kFrameLevel ? 7u : 6u); ++c) {
        out.push_back('\t');
        out.append(std::to_string(cols[c]));
      }
      if (consensus) {
        out.push_back('\t');
        for (uint32_t k = 0; k < x.length; ++k) {
          const uint8_t c = res.cons[x.offset + k];
          out.push_back(res.depth[x.offset + k] == 0 ? '.' : c < 25 ? kLetters[c] : '-');
        }
      }
      out.push_back('\n');
    }
  ReplaceText(&out);
}

// -y 8 and -y 9, from the -y 7 text FormatPathTabular left in the pieces (one
// line per hit, thirteen columns) and the hits' rows. -y 8 appends positives,
// the query row and the subject row to the line. -y 9 writes a block per hit:
// '#' and the first fourteen columns, then the three rows between their
// one-based first and last coordinates (columns 7 to 10 of the line), then an
// empty line.
void Session::FormatRows() {
  const std::vector<GhostmHitRows> &rows = HitsRows();
  const std::vector<GhostmHitPath> &path = hits_path_;
  const std::vector<uint8_t> &bytes = row_bytes_;
  const bool pairwise = opt_.output_style == 9;
  const auto extra = [&](size_t first, size_t n) {
    size_t need = n * 48;
    for (size_t i = 0; i < n; ++i) need += 3 * (size_t)rows[first + i].columns;
    return need;
  };
  RewriteLines("rows output", 0, extra,
               [&](size_t hit, const std::string &in, size_t pos, size_t nl, const size_t *, std::string &out) {
    const GhostmHitRows &x = rows[hit];
    const GhostmHitPath &p = path[hit];
    const char *q = reinterpret_cast<const char *>(bytes.data() + x.rows_offset);
    const size_t n = x.columns;
    char num[16], *end;
    if (pairwise) out.append("# ");
    out.append(in, pos, nl - pos);
    out.push_back('\t');
    end = PutU32(num, x.positives);
    out.append(num, (size_t)(end - num));
    if (!pairwise) {
      out.push_back('\t');
      out.append(q, n);
      out.push_back('\t');
      out.append(q + 2 * n, n);
      out.push_back('\n');
    } else {
      out.append("\nQuery\t");
      const uint32_t q0 = TileOffset(hit) + 1;  // a tiled set prints read coordinates
      end = PutU32(num, p.q_start + q0);
      out.append(num, (size_t)(end - num));
      out.push_back('\t');
      out.append(q, n);
      out.push_back('\t');
      end = PutU32(num, p.q_end + q0);
      out.append(num, (size_t)(end - num));
      out.append("\n\t\t");
      out.append(q + n, n);
      out.append("\t\nSbjct\t");
      end = PutU32(num, p.s_start + 1);
      out.append(num, (size_t)(end - num));
      out.push_back('\t');
      out.append(q + 2 * n, n);
      out.push_back('\t');
      end = PutU32(num, p.s_end + 1);
      out.append(num, (size_t)(end - num));
      out.append("\n\n");
    }
  });
}

// -y 6: qseqid sseqid pident length mismatch gapopen qstart qend sstart send
// evalue bitscore, tab-separated. Every piece holds the style-0 lines of its
// hits (name, name, pident, length, matches, start, end, E-value, bits, each
// followed by a tab): the line keeps everything up to the length, then the
// four new columns, then style 0's start, end, E-value and bit-score bytes.
// The fields are found from the line's end, so a tab inside a name is harmless.
void Session::FormatTabular() {
  const std::vector<GhostmHitExt> &ext = HitsExt();
  // tab[5]: the tab after the length
  RewriteLines("tabular output", 6, [](size_t, size_t n) { return n * 24; },
               [&](size_t hit, const std::string &in, size_t pos, size_t, const size_t *tab, std::string &out) {
    const GhostmHitExt &x = ext[hit];
    out.append(in, pos, tab[5] - pos);
    char num[64], *p = num;
    *p++ = '\t';
    p = PutU32(p, x.mismatches); *p++ = '\t';
    p = PutU32(p, x.gap_opens); *p++ = '\t';
    const uint32_t q0 = TileOffset(hit) + 1;  // a tiled set prints read coordinates
    p = PutU32(p, x.q_start + q0); *p++ = '\t';
    p = PutU32(p, x.q_end + q0); *p++ = '\t';
    out.append(num, (size_t)(p - num));
    out.append(in, tab[4] + 1, tab[0] - tab[4] - 1);
    out.push_back('\n');
  });
}

void Session::Part::Reset(size_t pieces) {
  text.resize(pieces);
  hits.resize(pieces);
  for (std::string &t : text) t.clear();
  for (std::vector<GhostmHit> &h : hits) h.clear();
  std::lock_guard<std::mutex> lk(mu);
  done.assign(pieces, 0);
  abandoned = false;
  streaming = false;
}

void Session::Part::MarkDone(size_t k) {
  {
    std::lock_guard<std::mutex> lk(mu);
    done[k] = 1;
  }
  cv.notify_all();
}

void Session::Part::Abandon() {
  {
    std::lock_guard<std::mutex> lk(mu);
    abandoned = true;
  }
  cv.notify_all();
}

bool Session::Part::Wait(size_t k) {
  std::unique_lock<std::mutex> lk(mu);
  cv.wait(lk, [&] { return done[k] || abandoned; });
  return done[k] != 0;
}

Session::Part *Session::NewPart() {
  if (used_parts_ == parts_.size()) parts_.emplace_back();
  return &parts_[used_parts_++];
}

void Session::FormatResults(const QueryData &q, const Results &results, Part *out) {
  const uint32_t n = q.chunk.nseq;
  out->Reset(threads_);
  const LineFormat &w = Format();
  ParallelFor(n, threads_, [&](size_t b, size_t e, unsigned t) {
    TextCursor text(out->text[t]);
    std::vector<GhostmHit> &hits = out->hits[t];
    for (size_t i = b; i < e; ++i) {
      const uint64_t space = (uint64_t)q.qlen[i] * (uint64_t)db_sum_u32_;
      const float scaled = (float)space * w.ev.p.K;
      const std::string_view qname = q.chunk.names[i];
      for (const HitRecord &h : results[i]) {
        const DbData &d = dbs_[h.db_chunk];
        const std::string_view sname = d.chunk.names[h.subject];
        char *p = text.Reserve(qname.size() + sname.size() + LineFormat::kFixed);
        text.Commit(w.Write(p, qname, sname, h.score, h.start, h.end, h.aln_len, h.aln_match, scaled, q.qlen[i]));
        hits.push_back(GhostmHit{q.global_base + (uint32_t)i, d.global_base + h.subject, h.score, h.start,
                                 h.end, h.aln_len, h.aln_match, h.seq_id});
      }
    }
  });
}

// Same text from the device-selected hits: a name group's lines are printed
// under its last query (the reference's result_list[last]).
void Session::FormatSelected(const QueryData &q, uint32_t g0, const std::vector<uint32_t> &counts,
                             const HostHits &hits, uint32_t cap, Part *out) {
  const uint32_t ng = (uint32_t)counts.size();
  const unsigned workers = std::max(1u, threads_ > 1 ? threads_ - 1 : 1u);
  // a streamed run cuts the part into four pieces per worker, formatted in
  // order, and the writer writes each as soon as it and those before it are
  // done (the file then trails the formatting by a piece, not by the part)
  const bool stream = stream_fd_ >= 0;
  const size_t pieces = PieceCount(ng, stream ? (size_t)workers * StreamPiecesPerWorker() : workers);
  out->Reset(pieces);
  struct AbandonOnError {  // a failed formatting releases the writer waiting for its pieces
    Part *p;
    bool armed = true;
    ~AbandonOnError() {
      if (armed) p->Abandon();
    }
  } abandon{out};
  if (stream) StreamPart(out);
  const LineFormat &w = Format();
  // timeline diagnostics: each worker's wall and on-CPU time (a thread that
  // waits for a CPU, e.g. under a cgroup quota, shows wall >> CPU)
  const bool trace = TraceOn();
  std::vector<double> wall(trace ? pieces : 0), cpu(trace ? pieces : 0);  // per piece
  ParallelForPieces(ng, pieces, workers, [&](size_t b, size_t e, unsigned t) {
    const double w0 = trace ? NowSeconds() : 0.0, c0 = trace ? ThreadCpuSeconds() : 0.0;
    struct Done {
      bool on;
      double w0, c0, *wall, *cpu;
      ~Done() {
        if (on) *wall = NowSeconds() - w0, *cpu = ThreadCpuSeconds() - c0;
      }
    } done{trace, w0, c0, trace ? &wall[t] : nullptr, trace ? &cpu[t] : nullptr};
    std::vector<GhostmHit> &ph = out->hits[t];
    size_t nh = 0;
    for (size_t g = b; g < e; ++g) nh += counts[g];
    out->text[t].reserve(nh * 96);
    ph.reserve(nh);
    {
    TextCursor text(out->text[t]);
    for (size_t g = b; g < e; ++g) {
      const uint32_t i = q.group_last[g0 + g];
      const std::string_view name = q.chunk.names[i];
      const uint64_t space = (uint64_t)q.qlen[i] * (uint64_t)db_sum_u32_;
      const float scaled = (float)space * w.ev.p.K;
      for (uint32_t k = 0; k < counts[g]; ++k) {
        const SelectedHit &h = hits[(size_t)g * cap + k];
        const DbData &d = dbs_[h.chunk];
        const uint32_t len = h.ml >> 8, match = h.ml & 0xFFu;
        const float seq_id = (float)match / (float)len;  // aligner.cpp:945
        const std::string_view sname = d.chunk.names[h.sid];
        char *p = text.Reserve(name.size() + sname.size() + LineFormat::kFixed);
        text.Commit(w.Write(p, name, sname, h.score, h.start, h.end, len, match, scaled, q.qlen[i]));
        ph.push_back(GhostmHit{q.global_base + i, d.global_base + h.sid, h.score, h.start, h.end, len, match,
                               seq_id});
      }
    }
    }  // the piece's text is final here (TextCursor trims it)
    if (stream) out->MarkDone(t);
  });
  abandon.armed = false;
  if (trace) {
    double ws = 0, cs = 0, wm = 0;
    for (size_t t = 0; t < pieces; ++t) ws += wall[t], cs += cpu[t], wm = std::max(wm, wall[t]);
    TraceMark("fmt_wall_max_us", (uint64_t)(wm * 1e6));
    TraceMark("fmt_wall_sum_us", (uint64_t)(ws * 1e6));
    TraceMark("fmt_cpu_sum_us", (uint64_t)(cs * 1e6));
  }
}

void Session::DropResults() {
  used_parts_ = 0;
  joined_.clear();
  joined_valid_ = false;
  hits_.clear();
  hits_valid_ = false;
  hits_ext_.clear();
  hits_ext_valid_ = false;
  hit_source_.clear();
  hits_path_.clear();
  path_ops_.clear();
  hits_path_valid_ = false;
  hits_rows_.clear();
  row_bytes_.clear();
  row_bytes_.shrink_to_fit();
  hits_rows_valid_ = false;
  DropLevel(0);
  DropLevel(1);
  pileup_subj_.clear();
  pileup_[kTileLevel].Drop();
}

void Session::Run(bool stream_to_file) {
  DeviceModule &dev = DeviceModule::Get();
  formatter_->Drain();
  if (writer_) writer_->Drain();
  streamed_ = false;
  stream_failed_ = false;
  stream_off_ = 0;
  // -y 6 to -y 27 are written after the post-pass (HitsExt, HitsPath, HitsRows, Pileup, HitsReadRows, ReadPileup,
  // ReadCull, ReadLca, TaxonProfile, PairLca), not while the search runs
  const bool tabular = opt_.output_style >= 6 && opt_.output_style <= 27;
  if (stream_to_file && !tabular) {
    if (!writer_) writer_ = std::make_unique<TaskQueue>();
    // an unwritable path writes nothing, as the reference's unchecked ofstream
    stream_fd_ = open(opt_.output_file.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  }
  struct CloseStream {  // also on an error: the formatter, then the writer drained, the file closed
    Session *s;
    ~CloseStream() {
      if (s->stream_fd_ < 0) return;
      // a formatting task still running may hand a part to the writer, which
      // must not reach a closed (or reused) descriptor
      try {
        s->formatter_->Drain();
      } catch (...) {
        s->stream_failed_ = true;
      }
      try {
        s->writer_->Drain();
      } catch (...) {
        s->stream_failed_ = true;
      }
      close(s->stream_fd_);
      s->stream_fd_ = -1;
    }
  } close_stream{this};
  dev.ResetTimes();
  stats_ = GhostmStats{};
  band_stats_ = GhostmBandStats{};
  frame_stats_ = GhostmFrameStats{};
  read_rows_stats_ = GhostmReadRowsStats{};
  read_pileup_stats_ = GhostmReadPileupStats{};
  cull_stats_ = GhostmReadCullStats{};
  lca_stats_ = GhostmReadLcaStats{};
  profile_stats_ = GhostmTaxonProfileStats{};
  pair_stats_ = GhostmPairJoinStats{};
  QueryStats();
  merge_epoch_ = 0;
  DropResults();
  Format();  // built here, before any formatting task can need it
  dev.ResetRecords(HitCapacity());  // the most records the run can append
  records_on_device_ = true;
  const double t0 = NowSeconds();
  TraceMark("run");
  // Both streams drained at the start of a run and after each chunk's carry
  // reset: without these waits (which find the streams idle, < 0.03 ms) a
  // session's second run waited 10-28 ms before its first K1 kernel
  // (profiles/r5i/). GHOSTM_RUN_SYNC=0 leaves them out (A/B).
  const char *rs = getenv("GHOSTM_RUN_SYNC");
  run_sync_ = !(rs && strcmp(rs, "0") == 0);
  if (run_sync_) dev.Synchronize();
  TraceMark("run_idle");
  for (QueryData &q : queries_) {
    if (dbs_.empty()) break;  // no database (yet): empty output, no hits
    RunQueryChunk(q);
    stats_.queries += q.chunk.nseq;
    for (uint32_t v : q.qlen) stats_.query_residues += v;
  }
  TraceMark("drain");
  formatter_->Drain();
  if (stream_fd_ >= 0) {
    writer_->Drain();
    TraceMark("streamed", stream_off_);
    if (stream_failed_) throw Error("writing " + opt_.output_file + " failed");
    streamed_ = true;
  }
  stats_.seconds_total = NowSeconds() - t0;
  TraceMark("run_end");
  TraceDump();
  const DeviceTimes &dt = dev.times();
  StageCounters(dt, &stats_);
  stats_.tracebacks += dt.traced_hits;  // device merge (the host merge counts its own)
  for (size_t k = 0; k < used_parts_; ++k)
    for (const auto &h : parts_[k].hits) stats_.hits += h.size();
  if (tabular) {
    if (opt_.output_style == 26 || opt_.output_style == 27) {
      FormatPairLca(opt_.output_style == 27);
    } else if (opt_.output_style == 24 || opt_.output_style == 25) {
      FormatProfile(opt_.output_style == 25);
    } else if (opt_.output_style == 22 || opt_.output_style == 23) {
      FormatLca(opt_.output_style == 23);
    } else if (opt_.output_style == 20 || opt_.output_style == 21) {
      if (opt_.output_style == 21) FormatFrameTabular();
      else FormatPathTabular(true);
      FormatCull(opt_.output_style == 21);
    } else if (opt_.output_style >= 16)
      FormatPileup(opt_.output_style >= 18 ? kFrameLevel : kBandLevel, opt_.output_style == 17 || opt_.output_style == 19);
    else if (opt_.output_style == 13 || opt_.output_style == 15) FormatFrameTabular();
    else if (opt_.output_style == 12 || opt_.output_style == 14) FormatPathTabular(true);
    else if (opt_.output_style >= 10) FormatPileup(kTileLevel, opt_.output_style == 11);
    else if (opt_.output_style == 6) FormatTabular();
    else FormatPathTabular();
    if (opt_.output_style == 8 || opt_.output_style == 9) FormatRows();
    if (opt_.output_style == 14 || opt_.output_style == 15) FormatReadRows(opt_.output_style == 15);
    if (stream_to_file) {
      WriteOutputFile();
      streamed_ = true;
    }
    stats_.seconds_total = NowSeconds() - t0;
  }
}

const std::string &Session::Output() {
  if (!joined_valid_) {
    size_t n = 0;
    for (size_t k = 0; k < used_parts_; ++k)
      for (const std::string &t : parts_[k].text) n += t.size();
    joined_.clear();
    joined_.reserve(n);
    for (size_t k = 0; k < used_parts_; ++k)
      for (const std::string &t : parts_[k].text) joined_.append(t);
    joined_valid_ = true;
  }
  return joined_;
}

const std::vector<GhostmHit> &Session::Hits() {
  if (!hits_valid_) {
    hits_.clear();
    for (size_t k = 0; k < used_parts_; ++k)
      for (const auto &h : parts_[k].hits) hits_.insert(hits_.end(), h.begin(), h.end());
    hits_valid_ = true;
  }
  return hits_;
}

uint64_t Session::HitCapacity() const {
  uint64_t n = 0;  // each name group keeps at most -b hits
  for (const QueryData &q : queries_) n += (uint64_t)q.group_first.size() * std::max<uint32_t>(opt_.best, 1);
  return n;
}

size_t Session::DeviceHits(void *dst, size_t cap) {
  DeviceModule &dev = DeviceModule::Get();
  if (!records_on_device_) {
    const std::vector<GhostmHit> &h = Hits();
    dev.UploadRecords(h.data(), h.size());
    records_on_device_ = true;
  }
  const size_t n = (size_t)dev.RecordCount();
  if (dst && cap) dev.CopyRecords(dst, std::min(n, cap));
  return n;
}

// The writer's task for a streamed part: piece k is written once it is
// formatted (Part::Wait), in order; submitted before the formatting starts, so
// the writer's tasks stay in part order.
void Session::StreamPart(Part *part) {
  part->streaming = true;
  writer_->Submit([this, part] {
    TraceMark("w_begin", stream_off_);
    struct Done {
      const uint64_t &off;
      ~Done() { TraceMark("w_end", off); }
    } done{stream_off_};
    for (size_t k = 0; k < part->text.size(); ++k) {
      if (!part->Wait(k)) return;  // formatting failed: the run throws from the formatter
      const char *p = part->text[k].data();
      size_t left = part->text[k].size();
      while (left && !stream_failed_) {
        const ssize_t w = pwrite(stream_fd_, p, left, (off_t)stream_off_);
        if (w <= 0) {
          stream_failed_ = true;
          break;
        }
        p += w;
        left -= (size_t)w;
        stream_off_ += (uint64_t)w;
      }
    }
  });
}

void Session::PartDone(const Part *part) {
  if (stream_fd_ < 0 || part->streaming) return;  // (a streamed part is written by StreamPart's task)
  writer_->Submit([this, part] {
    TraceMark("w_begin", stream_off_);
    struct Done {
      const uint64_t &off;
      ~Done() { TraceMark("w_end", off); }
    } done{stream_off_};
    for (const std::string &t : part->text) {
      const char *p = t.data();
      size_t left = t.size();
      while (left && !stream_failed_) {
        const ssize_t w = pwrite(stream_fd_, p, left, (off_t)stream_off_);
        if (w <= 0) {
          stream_failed_ = true;
          break;
        }
        p += w;
        left -= (size_t)w;
        stream_off_ += (uint64_t)w;
      }
    }
  });
}

void Session::WriteOutputFile() {
  if (streamed_) return;  // Run(true) wrote it while searching
  TraceMark("write");
  struct Done {
    ~Done() {
      TraceMark("written");
      TraceDump();
    }
  } done;
  // the pieces in output order, written at their offsets by parallel threads
  // (an unwritable path writes nothing, as the reference's unchecked ofstream)
  std::vector<const std::string *> pieces;
  std::vector<uint64_t> at;
  uint64_t total = 0;
  for (size_t k = 0; k < used_parts_; ++k)
    for (const std::string &t : parts_[k].text) {
      if (t.empty()) continue;
      pieces.push_back(&t);
      at.push_back(total);
      total += t.size();
    }
  const int fd = open(opt_.output_file.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) return;
  std::vector<char> failed(pieces.size(), 0);
  ParallelFor(pieces.size(), std::max<unsigned>(1u, std::min(threads_, 8u)), [&](size_t b, size_t e, unsigned) {
    for (size_t k = b; k < e; ++k) {
      const char *p = pieces[k]->data();
      size_t left = pieces[k]->size();
      off_t off = (off_t)at[k];
      while (left) {
        const ssize_t w = pwrite(fd, p, left, off);
        if (w <= 0) {
          failed[k] = 1;
          break;
        }
        p += w;
        off += w;
        left -= (size_t)w;
      }
    }
  });
  close(fd);
  for (char f : failed)
    if (f) throw Error("writing " + opt_.output_file + " failed");
}

// ------------------------------------------------------------------ query sets
// The session's queries replaced on the live session: what `ghostm qry` would
// write for the same records (query_set.h: the chunk cuts, the width rule) is
// made resident chunk by chunk by DeviceModule::FormatQuery, without .seq files
// and without the records visiting the host. The DB chunks, the matrix and the
// options stay as they are.
void Session::DropQueries() {
  if (shard_world_ > 1) throw Error("a shard session's query set cannot be replaced");
  if (formatter_) formatter_->Drain();
  if (writer_) writer_->Drain();
  DeviceModule &dev = DeviceModule::Get();
  dev.Synchronize();
  DropResults();
  dev.ResetRecords(0);
  records_on_device_ = true;
  streamed_ = false;
  stream_failed_ = false;
  stream_off_ = 0;
  seed_counts_.clear();
  seed_offsets_.clear();
  stats_ = GhostmStats{};
  // the old chunks' device blocks go back to the pool
  for (QueryData &q : queries_) dev.Free(q.dev);
  queries_.clear();
  tile_table_.clear();  // a tiled set's table goes with the set
  tile_read_nt_.clear();
  tile_step_ = 0;
  shard_begin_ = 0;
  shard_end_ = UINT64_MAX;
  format_seconds_ = 0;
  format_launches_ = 0;
  read_seconds_ = 0;
  load_seconds_ = 0;
  mask_stats_ = GhostmMaskStats{};
  qual_out_.clear();
  qual_stats_ = GhostmQualStats{};
  adapter_out_.clear();
  adapter_stats_ = GhostmAdapterStats{};
  QueryStats();
}

void Session::AddQueryChunk(const QueryRecordView *recs, uint32_t n, uint32_t width, bool dna, uint64_t *cut_records,
                            std::vector<std::string> *cut_names) {
  DeviceModule &dev = DeviceModule::Get();
  const double t0 = NowSeconds();
  const uint32_t per = dna ? 6 : 1;
  // every read is cut/padded to the chunk's first read length (query_creator.cpp:254)
  const uint32_t dna_len = dna ? recs[0].len : 0;
  // the letters a record can contribute, concatenated
  const uint32_t most = dna ? dna_len : width;
  std::vector<uint64_t> off(n);
  std::vector<uint32_t> len(n);
  uint64_t total = 0;
  for (uint32_t r = 0; r < n; ++r) {
    off[r] = total;
    len[r] = std::min(recs[r].len, most);
    total += len[r];
  }
  std::vector<uint8_t> raw(total);
  ParallelFor(n, std::max(1u, std::min(threads_, 8u)), [&](size_t b, size_t e, unsigned) {
    for (size_t r = b; r < e; ++r)
      if (len[r]) std::memcpy(raw.data() + off[r], recs[r].seq, len[r]);
  });
  QueryData q;
  q.chunk.id = (uint32_t)queries_.size();
  q.chunk.nseq = n * per;
  q.chunk.L = width;
  for (uint32_t r = 0; r < n; ++r) {
    // qry's over-width warning, per output record (frames: dna_len / 3 letters)
    const uint32_t letters = dna ? dna_len / 3 : recs[r].len;
    for (uint32_t k = 0; k < per; ++k) {
      q.chunk.names.push_back(recs[r].name);
      if (letters > width) {
        if (cut_records) ++*cut_records;
        if (cut_names) cut_names->emplace_back(recs[r].name);
      }
    }
  }
  PrepareQueryChunk(&q, false);
  q.qlen.assign(q.chunk.nseq, 1);
  double seconds = 0;
  q.dev = dev.FormatQuery(raw.data(), total, off.data(), len.data(), n, width, dna ? std::max(dna_len, 1u) : 0,
                          q.qlen.data(), &seconds);
  struct FreeUnadopted {
    QueryData *q;
    ~FreeUnadopted() {
      if (q) DeviceModule::Get().Free(q->dev);
    }
  } guard{&q};
  double mask_seconds = 0;
  if (mask_.window) {  // every record is its own source of `width` letters
    std::vector<GhostmBandSource> src(q.chunk.nseq);
    for (uint32_t i = 0; i < q.chunk.nseq; ++i) src[i] = GhostmBandSource{i, 1, 1, width};
    mask_seconds = MaskChunk(&q, src, width);
  }
  dev.SetQueryGroups(q.dev, q.group_first.data(), q.group_last.data(), (uint32_t)q.group_first.size());
  q.global_base = queries_.empty() ? 0 : queries_.back().global_base + queries_.back().chunk.nseq;
  format_seconds_ += seconds;
  ++format_launches_;
  queries_.push_back(std::move(q));
  guard.q = nullptr;
  load_seconds_ += NowSeconds() - t0 - seconds - mask_seconds;
}

void Session::FinishQuerySet() {
  ++query_sets_;
  QueryStats();
}

void Session::QueryStats() {
  stats_.seconds_query_format = format_seconds_;
  stats_.query_format_launches = format_launches_;
  stats_.query_sets = query_sets_;
  stats_.seconds_query_read = read_seconds_;
  stats_.seconds_query_load = load_seconds_;
}

namespace {
struct WidthRule {
  uint32_t width, max_concat;
};
WidthRule QuerySetRules(uint32_t width, bool dna, uint32_t chunk_mb, bool *capped) {
  bool c = false;
  WidthRule r{QueryRecordWidth(width, dna, &c), QueryChunkLimit(chunk_mb != 0, chunk_mb, dna)};
  if (capped) *capped = c;
  return r;
}
}  // namespace

void Session::SetQueries(const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets, const uint32_t *lengths,
                         const char *names, uint64_t names_len, uint32_t n, uint32_t width, bool dna,
                         uint32_t chunk_mb) {
  if (n && (!offsets || !lengths || !names || (!raw && raw_len))) throw Error("set queries: null argument");
  std::vector<QueryRecordView> recs(n);
  uint64_t at = 0;
  for (uint32_t r = 0; r < n; ++r) {
    if (offsets[r] > raw_len || lengths[r] > raw_len - offsets[r])
      throw Error("set queries: record " + std::to_string(r) + " outside the letter buffer");
    const char *nl = at < names_len ? static_cast<const char *>(std::memchr(names + at, '\n', names_len - at)) : nullptr;
    if (!nl) throw Error("set queries: fewer than " + std::to_string(n) + " newline-terminated names");
    recs[r] = QueryRecordView{reinterpret_cast<const char *>(raw) + offsets[r], lengths[r],
                              std::string_view(names + at, (size_t)(nl - (names + at)))};
    at = (uint64_t)(nl - names) + 1;
  }
  const WidthRule rule = QuerySetRules(width, dna, chunk_mb, nullptr);
  std::vector<uint64_t> cuts;
  const bool whole = QueryChunkCuts(lengths, n, rule.max_concat, &cuts);
  DropQueries();
  try {
    for (size_t c = 0; c + 1 < cuts.size(); ++c)
      AddQueryChunk(recs.data() + cuts[c], (uint32_t)(cuts[c + 1] - cuts[c]), rule.width, dna, nullptr, nullptr);
    if (!whole) throw Error("set queries: too small max length.");
  } catch (...) {
    DropQueries();  // no half-made set
    throw;
  }
  FinishQuerySet();
}

void Session::SetQueriesFasta(const std::string &path, uint32_t width, bool dna, uint32_t chunk_mb,
                              uint64_t *cut_records, std::vector<std::string> *cut_names, bool *capped) {
  const WidthRule rule = QuerySetRules(width, dna, chunk_mb, capped);
  if (cut_records) *cut_records = 0;
  {
    std::ifstream probe(path.c_str());
    if (!probe) throw Error("set queries: cannot open " + path);
  }
  DropQueries();
  try {
    QueryChunkReader reader(path, rule.max_concat);
    std::vector<FastaRecord> recs;
    std::vector<QueryRecordView> views;
    for (;;) {
      const double t0 = NowSeconds();
      const int more = reader.Next(&recs);
      read_seconds_ += NowSeconds() - t0;
      if (more < 0) throw Error("set queries: too small max length.");
      if (more == 0) break;
      views.resize(recs.size());
      for (size_t r = 0; r < recs.size(); ++r) {
        if (recs[r].seq.size() > UINT32_MAX) throw Error("set queries: a record of over 4 G letters");
        views[r] = QueryRecordView{recs[r].seq.data(), (uint32_t)recs[r].seq.size(), recs[r].name};
      }
      AddQueryChunk(views.data(), (uint32_t)views.size(), rule.width, dna, cut_records, cut_names);
    }
  } catch (...) {
    DropQueries();  // no half-made set
    throw;
  }
  FinishQuerySet();
}

// ------------------------------------------------------------------ tiled query sets
// A set whose records may be longer than the width: every record enters as
// overlapping tile records under its name (query_tiles.h), so the name group
// merges a read's tiles as it merges a DNA read's frames and the search behind
// the formatter runs unchanged. The whole set is planned on the host (chunk
// cuts over the kept letters, tile counts, the chunks' row counts) before the
// old set is dropped, so every refusal leaves the session as it was.
void Session::AddQueryChunkTiled(const QueryRecordView *recs, uint32_t n, uint32_t record_base,
                                 const TiledRule &rule) {
  DeviceModule &dev = DeviceModule::Get();
  const double t0 = NowSeconds();
  std::vector<uint64_t> off(n);
  std::vector<uint32_t> len(n), first(n + 1);
  std::vector<GhostmQueryTile> table;
  uint64_t total = 0;
  for (uint32_t r = 0; r < n; ++r) {
    off[r] = total;
    len[r] = recs[r].len;
    total += len[r];
    first[r] = (uint32_t)table.size();
    AppendTiles(record_base + r, len[r], rule.width, rule.dna, rule.step, &table);
  }
  first[n] = (uint32_t)table.size();
  CheckTiledChunk(table.size(), rule.width);
  std::vector<uint8_t> raw(total);
  ParallelFor(n, std::max(1u, std::min(threads_, 8u)), [&](size_t b, size_t e, unsigned) {
    for (size_t r = b; r < e; ++r)
      if (len[r]) std::memcpy(raw.data() + off[r], recs[r].seq, len[r]);
  });
  QueryData q;
  q.chunk.id = (uint32_t)queries_.size();
  q.chunk.nseq = first[n];
  q.chunk.L = rule.width;
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t k = first[r]; k < first[r + 1]; ++k) q.chunk.names.push_back(recs[r].name);
  PrepareQueryChunk(&q, false);
  if (tile_groups_) {  // a name group also ends where a tile begins: every record, or every six of a DNA set
    const uint32_t nrec = q.chunk.nseq;
    q.group_first.clear();
    q.group_last.clear();
    for (uint32_t i = nrec; i-- > 0;) {
      const bool tile_begins = i + 1 < nrec && (!rule.dna || table[i + 1].frame == 0);
      if (tile_begins) q.group_end[i] = i + 1;
      else if (i + 1 < nrec && q.group_end[i] != i + 1) q.group_end[i] = q.group_end[i + 1];
    }
    for (uint32_t i = 0; i < nrec; i = q.group_end[i]) {
      q.group_first.push_back(i);
      q.group_last.push_back(q.group_end[i] - 1);
    }
  }
  q.qlen.assign(q.chunk.nseq, 1);
  double seconds = 0;
  q.dev = dev.FormatQueryTiled(raw.data(), total, off.data(), len.data(), first.data(), n, rule.width, rule.dna,
                               rule.step, q.qlen.data(), &seconds);
  struct FreeUnadopted {
    QueryData *q;
    ~FreeUnadopted() {
      if (q) DeviceModule::Get().Free(q->dev);
    }
  } guard{&q};
  double mask_seconds = 0;
  if (mask_.window) {  // a protein record's kept letters, or each of a read's six frames (tiles six records apart)
    const uint32_t per = rule.dna ? 6 : 1;
    std::vector<GhostmBandSource> src;
    src.reserve((size_t)n * per);
    for (uint32_t r = 0; r < n; ++r) {
      const uint32_t m = rule.dna ? len[r] / 3 : len[r];
      if (m < mask_.window) continue;  // left alone (and a source needs a letter)
      const uint32_t tiles = TileCount(m, rule.width, rule.step);
      for (uint32_t f = 0; f < per; ++f) src.push_back(GhostmBandSource{first[r] + f, per, tiles, m});
    }
    mask_seconds = MaskChunk(&q, src, rule.step);
  }
  dev.SetQueryGroups(q.dev, q.group_first.data(), q.group_last.data(), (uint32_t)q.group_first.size());
  q.global_base = queries_.empty() ? 0 : queries_.back().global_base + queries_.back().chunk.nseq;
  if ((uint64_t)q.global_base + q.chunk.nseq > UINT32_MAX) throw Error("set queries: over 4 G tile records");
  tile_table_.insert(tile_table_.end(), table.begin(), table.end());
  tile_read_nt_.resize(std::max<size_t>(tile_read_nt_.size(), (size_t)record_base + n));
  std::copy(len.begin(), len.end(), tile_read_nt_.begin() + record_base);
  format_seconds_ += seconds;
  ++format_launches_;
  queries_.push_back(std::move(q));
  guard.q = nullptr;
  load_seconds_ += NowSeconds() - t0 - seconds - mask_seconds;
}

void Session::SetTiledRecords(const QueryRecordView *recs, uint32_t n, const TiledRule &rule) {
  if (shard_world_ > 1) throw Error("a shard session's query set cannot be replaced");
  CheckTileStep(rule.width, rule.step);
  std::vector<uint32_t> len(n);
  for (uint32_t r = 0; r < n; ++r) len[r] = recs[r].len;
  std::vector<uint64_t> cuts;
  const bool whole = QueryChunkCuts(len.data(), n, rule.max_concat, &cuts);
  if (!whole || cuts.back() != n) throw Error("set queries: too small max length.");
  uint64_t all = 0;
  for (size_t c = 0; c + 1 < cuts.size(); ++c) {
    uint64_t rows = 0;
    for (uint64_t r = cuts[c]; r < cuts[c + 1]; ++r)
      rows += AppendTiles((uint32_t)r, len[r], rule.width, rule.dna, rule.step, nullptr);
    CheckTiledChunk(rows, rule.width);
    all += rows;
  }
  if (all > UINT32_MAX) throw Error("set queries: over 4 G tile records");
  DropQueries();
  try {
    for (size_t c = 0; c + 1 < cuts.size(); ++c)
      AddQueryChunkTiled(recs + cuts[c], (uint32_t)(cuts[c + 1] - cuts[c]), (uint32_t)cuts[c], rule);
    tile_step_ = rule.step;
    tile_dna_ = rule.dna;
  } catch (...) {
    DropQueries();  // no half-made set
    throw;
  }
  FinishQuerySet();
}

void Session::SetQueriesTiled(const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets, const uint32_t *lengths,
                              const char *names, uint64_t names_len, uint32_t n, uint32_t width, bool dna,
                              uint32_t chunk_mb, uint32_t max_len, uint32_t step, uint64_t *cut_records) {
  if (n && (!offsets || !lengths || !names || (!raw && raw_len))) throw Error("set queries: null argument");
  if (cut_records) *cut_records = 0;
  std::vector<QueryRecordView> recs(n);
  uint64_t at = 0, cut = 0;
  for (uint32_t r = 0; r < n; ++r) {
    if (offsets[r] > raw_len || lengths[r] > raw_len - offsets[r])
      throw Error("set queries: record " + std::to_string(r) + " outside the letter buffer");
    const char *nl = at < names_len ? static_cast<const char *>(std::memchr(names + at, '\n', names_len - at)) : nullptr;
    if (!nl) throw Error("set queries: fewer than " + std::to_string(n) + " newline-terminated names");
    const uint32_t kept = TileKept(lengths[r], max_len);
    cut += kept < lengths[r] ? (dna ? 6 : 1) : 0;
    recs[r] = QueryRecordView{reinterpret_cast<const char *>(raw) + offsets[r], kept,
                              std::string_view(names + at, (size_t)(nl - (names + at)))};
    at = (uint64_t)(nl - names) + 1;
  }
  const WidthRule rule = QuerySetRules(width, dna, chunk_mb, nullptr);
  SetTiledRecords(recs.data(), n, TiledRule{rule.width, rule.max_concat, step, dna});
  if (cut_records) *cut_records = cut;
}

void Session::SetQueriesFastaTiled(const std::string &path, uint32_t width, bool dna, uint32_t chunk_mb,
                                   uint32_t max_len, uint32_t step, uint64_t *cut_records, bool *capped) {
  SetFastaTiled(path, nullptr, width, dna, chunk_mb, max_len, step, cut_records, capped);
}

void Session::SetQueriesFastaMatesTiled(const std::string &path1, const std::string &path2, uint32_t width, bool dna,
                                        uint32_t chunk_mb, uint32_t max_len, uint32_t step, uint64_t *cut_records,
                                        bool *capped) {
  SetFastaTiled(path1, &path2, width, dna, chunk_mb, max_len, step, cut_records, capped);
}

void Session::SetFastaTiled(const std::string &path, const std::string *path2, uint32_t width, bool dna,
                            uint32_t chunk_mb, uint32_t max_len, uint32_t step, uint64_t *cut_records, bool *capped) {
  const WidthRule rule = QuerySetRules(width, dna, chunk_mb, capped);
  if (cut_records) *cut_records = 0;
  if (shard_world_ > 1) throw Error("a shard session's query set cannot be replaced");
  CheckTileStep(rule.width, step);
  for (const std::string *p : {&path, path2}) {
    if (!p) continue;
    std::ifstream probe(p->c_str());
    if (!probe) throw Error("set queries: cannot open " + *p);
  }
  const double t0 = NowSeconds();
  std::vector<FastaRecord> recs;
  {
    FastaReader reader(path);
    FastaRecord r;
    while (reader.Next(&r)) recs.push_back(r);
  }
  if (path2) {  // the mates' file: record i of each file side by side
    std::vector<FastaRecord> second;
    FastaReader reader(*path2);
    FastaRecord r;
    while (reader.Next(&r)) second.push_back(r);
    if (second.size() != recs.size())
      throw Error("set queries: mates: " + path + " has " + std::to_string(recs.size()) + " records, " + *path2 + " has " +
                  std::to_string(second.size()));
    std::vector<FastaRecord> both;
    both.reserve(2 * recs.size());
    for (size_t i = 0; i < recs.size(); ++i) {
      both.push_back(std::move(recs[i]));
      both.push_back(std::move(second[i]));
    }
    recs.swap(both);
  }
  if (recs.size() > UINT32_MAX) throw Error("set queries: over 4 G records");
  std::vector<QueryRecordView> views(recs.size());
  uint64_t cut = 0;
  for (size_t r = 0; r < recs.size(); ++r) {
    if (recs[r].seq.size() > UINT32_MAX) throw Error("set queries: a record of over 4 G letters");
    const uint32_t kept = TileKept((uint32_t)recs[r].seq.size(), max_len);
    cut += kept < recs[r].seq.size() ? (dna ? 6 : 1) : 0;
    views[r] = QueryRecordView{recs[r].seq.data(), kept, recs[r].name};
  }
  const double read = NowSeconds() - t0;
  SetTiledRecords(views.data(), (uint32_t)views.size(), TiledRule{rule.width, rule.max_concat, step, dna});
  read_seconds_ = read;
  QueryStats();
  if (cut_records) *cut_records = cut;
}

// ------------------------------------------------------------------ reads with qualities
// FASTQ files and the letters form with quality bytes take the tiled path: the
// adapter stage (read_adapter.h) and then the quality stage (read_quality.h) run
// on all reads before anything of the old set is touched, then each read's kept
// stretch is what SetTiledRecords sees.
void Session::SetQualTiled(FastqSet *a, FastqSet *b, uint32_t width, bool dna, uint32_t chunk_mb, uint32_t max_len,
                           uint32_t step, uint64_t *cut_records, bool *capped, double read_seconds) {
  const WidthRule rule = QuerySetRules(width, dna, chunk_mb, capped);
  if (cut_records) *cut_records = 0;
  if (shard_world_ > 1) throw Error("a shard session's query set cannot be replaced");
  CheckTileStep(rule.width, step);
  if (b && b->len.size() != a->len.size())
    throw Error("set queries: mates: the first file has " + std::to_string(a->len.size()) + " records, the second has " +
                std::to_string(b->len.size()));
  const size_t per = b ? 2 : 1, total = a->len.size() * per;
  if (total > UINT32_MAX) throw Error("set queries: over 4 G records");
  // the adapter stage first, over the whole set in the records' order: records 2i and 2i + 1 are mates
  const AdapterParams adapters = adapter_;
  std::vector<GhostmAdapterOut> cuts;
  GhostmAdapterStats adapter_sum{};
  std::vector<uint32_t> cut_len[2];  // the reads' lengths from here on
  if (adapters.On()) {
    if (!dna) throw Error("adapters: a protein set");
    if (adapters.pair_overlap && (total & 1))
      throw Error("adapters: pairs: " + std::to_string(total) + " records are no whole pairs");
    std::vector<const uint8_t *> reads(total);
    std::vector<uint32_t> lens(total);
    for (size_t r = 0; r < total; ++r) {
      const FastqSet &f = r % per ? *b : *a;
      const size_t i = r / per;
      if (f.off[i] > f.letters.size() || f.len[i] > f.letters.size() - f.off[i])
        throw Error("adapters: record: read " + std::to_string(r) + " outside the letters given");
      if (f.len[i] > kAdapterLengthMax) throw Error("adapters: length: read " + std::to_string(r) + " has over 2^24 letters");
      reads[r] = reinterpret_cast<const uint8_t *>(f.letters.data()) + f.off[i];
      lens[r] = f.len[i];
    }
    cuts.resize(total);
    if (total) DeviceModule::Get().AdapterTrim(reads.data(), lens.data(), (uint32_t)total, adapters, cuts.data(), &adapter_sum);
    for (size_t k = 0; k < per; ++k) cut_len[k].resize(a->len.size());
    for (size_t r = 0; r < total; ++r) cut_len[r % per][r / per] = cuts[r].kept;
  }
  const QualParams params = qual_;
  std::vector<GhostmQualOut> outs[2];
  GhostmQualStats sum{};
  for (size_t k = 0; k < per; ++k) {
    FastqSet &f = k ? *b : *a;
    const uint32_t n = (uint32_t)f.len.size();
    const uint32_t *lens = adapters.On() ? cut_len[k].data() : f.len.data();
    outs[k].resize(n);
    uint8_t *letters = reinterpret_cast<uint8_t *>(&f.letters[0]);
    const uint8_t *qual = reinterpret_cast<const uint8_t *>(f.qual.data());
    const std::string why = ValidateQuality(letters, qual, f.letters.size(), f.off.data(), lens, n, params.trim_q,
                                            params.mask_q, params.min_len, outs[k].data());
    if (!why.empty()) throw Error("quality: " + why);
    if (!params.On() || n == 0) continue;
    GhostmQualStats one{};
    DeviceModule::Get().QualityTrim(letters, qual, f.off.data(), lens, n, params, outs[k].data(), &one);
    for (uint32_t r = 0; r < n; ++r)
      if (outs[k][r].bad) throw Error("fastq: record " + std::to_string(r + 1) + ": quality byte outside '!'..'~'");
    sum.launches += one.launches;
    sum.reads += one.reads;
    sum.letters += one.letters;
    sum.trimmed5 += one.trimmed5;
    sum.trimmed3 += one.trimmed3;
    sum.masked += one.masked;
    sum.failed += one.failed;
    sum.bad += one.bad;
    sum.seconds_quality += one.seconds_quality;
  }
  std::vector<QueryRecordView> views(total);
  std::vector<GhostmQualOut> all;
  if (params.On()) all.resize(total);
  uint64_t cut = 0;
  for (size_t r = 0; r < total; ++r) {
    const FastqSet &f = r % per ? *b : *a;
    const size_t i = r / per;
    uint32_t begin = 0, len = adapters.On() ? cuts[r].kept : f.len[i];
    if (params.On()) {
      all[r] = outs[r % per][i];
      begin = all[r].begin;
      len = all[r].kept;
    }
    const uint32_t kept = TileKept(len, max_len);
    cut += kept < len ? (dna ? 6 : 1) : 0;
    views[r] = QueryRecordView{f.letters.data() + f.off[i] + begin, kept, f.names[i]};
  }
  SetTiledRecords(views.data(), (uint32_t)views.size(), TiledRule{rule.width, rule.max_concat, step, dna});
  qual_out_.swap(all);
  qual_stats_ = sum;
  adapter_out_.swap(cuts);
  adapter_stats_ = adapter_sum;
  read_seconds_ = read_seconds;
  QueryStats();
  if (cut_records) *cut_records = cut;
}

void Session::SetQueriesFastqTiled(const std::string &path, uint32_t width, bool dna, uint32_t chunk_mb,
                                   uint32_t max_len, uint32_t step, uint64_t *cut_records, bool *capped) {
  const double t0 = NowSeconds();
  FastqSet a;
  try {
    ReadFastqSet(path, &a);
  } catch (FastqError &e) {
    throw Error(e.what());
  }
  SetQualTiled(&a, nullptr, width, dna, chunk_mb, max_len, step, cut_records, capped, NowSeconds() - t0);
}

void Session::SetQueriesFastqMatesTiled(const std::string &path1, const std::string &path2, uint32_t width, bool dna,
                                        uint32_t chunk_mb, uint32_t max_len, uint32_t step, uint64_t *cut_records,
                                        bool *capped) {
  const double t0 = NowSeconds();
  FastqSet a, b;
  try {
    ReadFastqSet(path1, &a);
    ReadFastqSet(path2, &b);
  } catch (FastqError &e) {
    throw Error(e.what());
  }
  if (a.len.size() != b.len.size())
    throw Error("set queries: mates: " + path1 + " has " + std::to_string(a.len.size()) + " records, " + path2 + " has " +
                std::to_string(b.len.size()));
  SetQualTiled(&a, &b, width, dna, chunk_mb, max_len, step, cut_records, capped, NowSeconds() - t0);
}

void Session::SetQueriesQualTiled(const uint8_t *raw, const uint8_t *qual, uint64_t raw_len, const uint64_t *offsets,
                                  const uint32_t *lengths, const char *names, uint64_t names_len, uint32_t n,
                                  uint32_t width, bool dna, uint32_t chunk_mb, uint32_t max_len, uint32_t step,
                                  uint64_t *cut_records) {
  if (n && (!offsets || !lengths || !names || ((!raw || !qual) && raw_len))) throw Error("set queries: null argument");
  FastqSet a;  // a copy: the caller's letters are not changed
  a.off.assign(offsets, offsets + n);
  a.len.assign(lengths, lengths + n);
  a.names.resize(n);
  uint64_t at = 0;
  for (uint32_t r = 0; r < n; ++r) {
    if (offsets[r] > raw_len || lengths[r] > raw_len - offsets[r])
      throw Error("set queries: record " + std::to_string(r) + " outside the letter buffer");
    const char *nl = at < names_len ? static_cast<const char *>(std::memchr(names + at, '\n', names_len - at)) : nullptr;
    if (!nl) throw Error("set queries: fewer than " + std::to_string(n) + " newline-terminated names");
    a.names[r].assign(names + at, (size_t)(nl - (names + at)));
    at = (uint64_t)(nl - names) + 1;
  }
  if (raw_len) {
    a.letters.assign(reinterpret_cast<const char *>(raw), raw_len);
    a.qual.assign(reinterpret_cast<const char *>(qual), raw_len);
  }
  SetQualTiled(&a, nullptr, width, dna, chunk_mb, max_len, step, cut_records, nullptr, 0);
}

// ------------------------------------------------------------------ database sets
// The session's database replaced on the live session: what `ghostm db` would
// write for the same records (db_set.h: the chunk cuts) is made resident chunk
// by chunk by DeviceModule::FormatDb, coded and indexed on the device, without
// files. The query chunks, the matrix and the options stay as they are.
void Session::DropDb() {
  if (shard_world_ > 1) throw Error("a shard session's database cannot be replaced: its batch plan was agreed on it");
  if (formatter_) formatter_->Drain();
  if (writer_) writer_->Drain();
  DeviceModule &dev = DeviceModule::Get();
  dev.Synchronize();
  DropResults();
  dev.ResetRecords(0);
  records_on_device_ = true;
  streamed_ = false;
  stream_failed_ = false;
  stream_off_ = 0;
  seed_counts_.clear();
  seed_offsets_.clear();
  stats_ = GhostmStats{};
  // the old chunks' device blocks go back to the pool
  for (DbData &d : dbs_) dev.Free(d.dev);
  dbs_.clear();
  tax_ = Taxonomy();  // its subjects are gone
  db_sum_u32_ = 0;
  // the E-value text cache is keyed by (query length, score) and was priced
  // with the old database's residue sum
  format_.reset();
  dev.SetChunkBases(nullptr, 0);
  db_format_seconds_ = 0;
  db_code_seconds_ = 0;
  db_format_launches_ = 0;
  db_read_seconds_ = 0;
  db_load_seconds_ = 0;
  QueryStats();
}

void Session::AddDbChunk(const QueryRecordView *recs, uint32_t n, uint32_t seed) {
  DeviceModule &dev = DeviceModule::Get();
  const double t0 = NowSeconds();
  // every record's letters followed by the separator (kernels.h k_db_code)
  std::vector<uint32_t> len(n), starts(n);
  uint64_t total = 0;
  for (uint32_t r = 0; r < n; ++r) {
    starts[r] = (uint32_t)total;
    len[r] = recs[r].len;
    total += (uint64_t)len[r] + 1;
  }
  if (total > UINT32_MAX) throw Error("set db: a chunk of over 4 G bytes");
  std::vector<uint8_t> packed(total);
  ParallelFor(n, std::max(1u, std::min(threads_, 8u)), [&](size_t b, size_t e, unsigned) {
    for (size_t r = b; r < e; ++r) {
      uint8_t *dst = packed.data() + starts[r];
      if (len[r]) std::memcpy(dst, recs[r].seq, len[r]);
      // a letter equal to the separator (records given in memory only) is any
      // other unknown letter: X
      for (uint8_t *p = dst; (p = static_cast<uint8_t *>(std::memchr(p, '\n', (size_t)(dst + len[r] - p)))); ++p)
        *p = '?';
      dst[len[r]] = '\n';
    }
  });
  DbData d;
  d.chunk.id = (uint32_t)dbs_.size();
  d.chunk.nseq = n;
  d.chunk.len = (uint32_t)total;
  d.chunk.seed = seed;
  d.chunk.kcl = (1u << (kCharBits * SeedWeight(seed))) + 1;
  for (uint32_t r = 0; r < n; ++r) d.chunk.names.push_back(recs[r].name);
  double code_s = 0, index_s = 0;
  d.dev = dev.FormatDb(packed.data(), (uint32_t)total, len.data(), n, seed, &d.chunk.npos, &code_s, &index_s);
  struct FreeUnadopted {
    DbData *d;
    ~FreeUnadopted() {
      if (d) DeviceModule::Get().Free(d->dev);
    }
  } guard{&d};
  dev.SetDbSubjects(d.dev, starts.data(), n);
  d.chunk.starts = std::move(starts);
  d.global_base = dbs_.empty() ? 0 : dbs_.back().global_base + dbs_.back().chunk.nseq;
  db_sum_u32_ += (uint32_t)(total - n);  // DBReader::GetSumDbLength() truncates to u32
  db_format_seconds_ += code_s + index_s;
  db_code_seconds_ += code_s;
  ++db_format_launches_;
  dbs_.push_back(std::move(d));
  guard.d = nullptr;
  db_load_seconds_ += NowSeconds() - t0 - code_s - index_s;
}

void Session::FinishDbSet() {
  std::vector<uint32_t> bases;
  for (const DbData &d : dbs_) bases.push_back(d.global_base);
  DeviceModule::Get().SetChunkBases(bases.data(), (uint32_t)bases.size());
  ++db_sets_;
}

GhostmDbSetStats Session::DbSetStats() const {
  GhostmDbSetStats st{};
  st.seconds_db_format = db_format_seconds_;
  st.seconds_db_code = db_code_seconds_;
  st.db_format_launches = db_format_launches_;
  st.db_sets = db_sets_;
  st.seconds_db_read = db_read_seconds_;
  st.seconds_db_load = db_load_seconds_;
  return st;
}

void Session::RefuseDbSet(uint32_t k, uint32_t chunk_mb) const {
  if (shard_world_ > 1) throw Error("a shard session's database cannot be replaced: its batch plan was agreed on it");
  if (k == 0 || k > 6) throw Error("set db: k = " + std::to_string(k) + " outside 1..6 (the index's seed weights)");
  if (chunk_mb > kDbChunkMbMax) throw Error("set db: chunk size above " + std::to_string(kDbChunkMbMax) + " MiB");
}

void Session::SetDb(const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets, const uint32_t *lengths,
                    const char *names, uint64_t names_len, uint32_t n, uint32_t k, uint32_t chunk_mb) {
  if (n && (!offsets || !lengths || !names || (!raw && raw_len))) throw Error("set db: null argument");
  RefuseDbSet(k, chunk_mb);
  std::vector<QueryRecordView> recs(n);
  uint64_t at = 0;
  for (uint32_t r = 0; r < n; ++r) {
    if (offsets[r] > raw_len || lengths[r] > raw_len - offsets[r])
      throw Error("set db: record " + std::to_string(r) + " outside the letter buffer");
    const char *nl = at < names_len ? static_cast<const char *>(std::memchr(names + at, '\n', names_len - at)) : nullptr;
    if (!nl) throw Error("set db: fewer than " + std::to_string(n) + " newline-terminated names");
    recs[r] = QueryRecordView{reinterpret_cast<const char *>(raw) + offsets[r], lengths[r],
                              std::string_view(names + at, (size_t)(nl - (names + at)))};
    at = (uint64_t)(nl - names) + 1;
  }
  std::vector<uint64_t> cuts;
  if (!DbChunkCuts(lengths, n, DbChunkLimit(chunk_mb), &cuts)) throw Error("set db: too small max length.");
  const uint32_t seed = (1u << k) - 1;
  DropDb();
  try {
    for (size_t c = 0; c + 1 < cuts.size(); ++c)
      AddDbChunk(recs.data() + cuts[c], (uint32_t)(cuts[c + 1] - cuts[c]), seed);
  } catch (...) {
    DropDb();  // no half-made database
    throw;
  }
  FinishDbSet();
}

void Session::SetDbFasta(const std::string &path, uint32_t k, uint32_t chunk_mb) {
  RefuseDbSet(k, chunk_mb);
  {
    std::ifstream probe(path.c_str());
    if (!probe) throw Error("set db: cannot open " + path);
  }
  const uint32_t seed = (1u << k) - 1;
  DropDb();
  try {
    DbChunkReader reader(path, DbChunkLimit(chunk_mb));
    std::vector<FastaRecord> recs;
    std::vector<QueryRecordView> views;
    for (;;) {
      const double t0 = NowSeconds();
      const int more = reader.Next(&recs);
      db_read_seconds_ += NowSeconds() - t0;
      if (more < 0) throw Error("set db: too small max length.");
      if (more == 0) break;
      views.resize(recs.size());
      for (size_t r = 0; r < recs.size(); ++r) {
        if (recs[r].seq.size() >= UINT32_MAX) throw Error("set db: a record of over 4 G letters");
        views[r] = QueryRecordView{recs[r].seq.data(), (uint32_t)recs[r].seq.size(), recs[r].name};
      }
      AddDbChunk(views.data(), (uint32_t)views.size(), seed);
    }
  } catch (...) {
    DropDb();  // no half-made database
    throw;
  }
  FinishDbSet();
}

void Session::DbChunkInfo(uint32_t chunk, GhostmDbChunkInfo *info) const {
  if (chunk >= dbs_.size()) throw Error("DB chunk " + std::to_string(chunk) + " of " + std::to_string(dbs_.size()));
  const DbChunk &c = dbs_[chunk].chunk;
  *info = GhostmDbChunkInfo{c.id, c.nseq, c.len, c.seed, c.kcl, c.npos};
}

size_t Session::DbRecords(uint32_t chunk, uint8_t *codes, size_t cap) {
  if (chunk >= dbs_.size()) throw Error("DB chunk " + std::to_string(chunk) + " of " + std::to_string(dbs_.size()));
  const size_t n = dbs_[chunk].chunk.len;
  if (!codes) return n;
  DeviceModule &dev = DeviceModule::Get();
  if (cap >= n) {
    dev.DownloadDb(dbs_[chunk].dev, codes, nullptr, nullptr);
    return n;
  }
  std::vector<uint8_t> all(n);
  dev.DownloadDb(dbs_[chunk].dev, all.data(), nullptr, nullptr);
  std::memcpy(codes, all.data(), cap);
  return cap;
}

void Session::DbIndex(uint32_t chunk, uint32_t *keys_count, size_t kc_cap, uint32_t *positions, size_t pos_cap) {
  if (chunk >= dbs_.size()) throw Error("DB chunk " + std::to_string(chunk) + " of " + std::to_string(dbs_.size()));
  const DbChunk &c = dbs_[chunk].chunk;
  if ((keys_count && kc_cap < c.kcl) || (positions && pos_cap < c.npos))
    throw Error("DB index: the arrays need " + std::to_string(c.kcl) + " and " + std::to_string(c.npos) + " words");
  DeviceModule::Get().DownloadDb(dbs_[chunk].dev, nullptr, keys_count, positions);
}

void Session::SetOutputFile(const std::string &path) {
  if (formatter_) formatter_->Drain();
  if (writer_) writer_->Drain();
  opt_.output_file = path;
  streamed_ = false;  // the last run's text has not been written to this file
}

std::vector<uint32_t> Session::AllQueryLengths() const {
  std::vector<uint32_t> out;
  for (const QueryData &q : queries_) out.insert(out.end(), q.qlen.begin(), q.qlen.end());
  return out;
}

size_t Session::QueryRecords(uint32_t chunk, uint8_t *codes, size_t cap) {
  if (chunk >= queries_.size()) throw Error("query chunk " + std::to_string(chunk) + " of " + std::to_string(queries_.size()));
  DeviceModule &dev = DeviceModule::Get();
  const size_t n = dev.QueryBytes(queries_[chunk].dev);
  if (!codes) return n;
  if (cap >= n) {
    dev.DownloadQuery(queries_[chunk].dev, codes);
    return n;
  }
  std::vector<uint8_t> all(n);
  dev.DownloadQuery(queries_[chunk].dev, all.data());
  std::memcpy(codes, all.data(), cap);
  return cap;
}

// defined after LineFormat (a complete type for format_)
Session::~Session() {
  formatter_.reset();
  DeviceModule &dev = DeviceModule::Get();
  for (QueryData &q : queries_) dev.Free(q.dev);
  for (DbData &d : dbs_) dev.Free(d.dev);
}

}  // namespace ghostm
