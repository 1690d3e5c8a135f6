// The host model of the read-level aligned rows (ghostm_amd/csrc/read_rows_host.cpp,
// included here so that the program stands alone) on random well-formed paths:
// sources of 1 to 400 letters laid out as tile records the way the tiled
// setters lay them out (protein tiles one after the other, a strand's frames
// six records apart), band and frame paths walked at random inside the bounds,
// and the rows, the counts and the rescore against a walk over the plain letter
// arrays written out here. Then the refusals: every output keeps its canary.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

namespace ghostm {
static std::string g_last;
void SetLastErrorMessage(const std::string &m) { g_last = m; }
}  // namespace ghostm

#include "../../ghostm_amd/csrc/read_rows_host.cpp"

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    return 1;            \
  } while (0)

using namespace ghostm;

static const char kAbc[] = "ARNDCQEGHILKMFPSTWYVBJZX*";
static char Show(uint8_t c) { return c < 25 ? kAbc[c] : '?'; }

struct Chunk {
  uint32_t W, step;
  std::vector<uint8_t> qseq;                       // records of W codes
  std::vector<std::vector<uint8_t>> plain;         // per source: its frames' letters, frame-major (1 or 3 frames)
  std::vector<GhostmBandSource> src;
  std::vector<uint32_t> frames;                    // 1 or 3
};

// a source of `frames` frames of m letters appended to the chunk
static void AddSource(std::mt19937 &rng, Chunk *c, uint32_t m, uint32_t frames) {
  const uint32_t tiles = TileCount(m, c->W, c->step), per = frames == 3 ? 6 : 1;
  const uint32_t first = (uint32_t)(c->qseq.size() / c->W) + (frames == 3 ? 3 * (rng() % 2) : 0);
  std::vector<uint8_t> plain((size_t)frames * m);
  for (uint8_t &x : plain) x = (uint8_t)(rng() % 8 ? rng() % 25 : rng() % 32);
  const size_t base = c->qseq.size();
  c->qseq.resize(base + (size_t)tiles * per * c->W, 23);
  for (uint32_t t = 0; t < tiles; ++t)
    for (uint32_t g = 0; g < frames; ++g) {
      const uint32_t start = TileStart(t, tiles, m, c->W, c->step);
      const size_t rec = first + g + (size_t)per * t;
      for (uint32_t k = 0; k < c->W && start + k < m; ++k) c->qseq[rec * c->W + k] = plain[(size_t)g * m + start + k];
    }
  c->plain.push_back(plain);
  c->src.push_back(GhostmBandSource{first, tiles > 1 ? per : (uint32_t)(rng() % 9), tiles, m});
  c->frames.push_back(frames);
}

int main() {
  std::mt19937 rng(20261020);
  int M[32 * 32];
  for (int &x : M) x = (int)(rng() % 16) - 8;
  std::vector<uint8_t> db(900);
  for (uint8_t &x : db) x = (uint8_t)(rng() % 8 ? rng() % 25 : rng() % 32);
  int trials = 0;
  for (int round = 0; round < 60; ++round) {
    const bool frame = round % 2;
    Chunk c;
    c.W = round % 3 ? 127 : 63;
    c.step = round % 5 == 0 ? c.W : round % 5 == 1 ? 1 : 1 + rng() % c.W;
    const uint32_t lens[] = {1, 5, c.W, c.W + 1, 200, 1 + (uint32_t)(rng() % 400)};
    for (uint32_t m : lens) AddSource(rng, &c, m, frame ? 3 : 1);
    const uint32_t nq = (uint32_t)(c.qseq.size() / c.W);
    const int open = -11, ext = -1, shift = -(int)(rng() % 20);
    // random paths with the text, counts and score expected of them
    std::vector<GhostmBandSource> src;
    std::vector<GhostmHitPath> rec;
    std::vector<uint32_t> ops;
    std::vector<std::string> want;
    std::vector<GhostmHitReadRows> want_rec;
    for (int h = 0; h < 40; ++h) {
      const size_t si = rng() % c.src.size();
      const int64_t m = c.src[si].letters, limit = frame ? 3 * m : m, unit = frame ? 3 : 1;
      int64_t p = rng() % limit;
      uint32_t s = rng() % 300;
      GhostmHitPath x{(uint32_t)p, 0, s, 0, 0, 0, ops.size()};
      std::string q, mid, sub;
      GhostmHitReadRows w{0, 0, 0, 0, 0, 0, 0, 0, 0};
      const int nwords = h % 7 == 0 ? 0 : 1 + rng() % (h % 5 == 0 ? 150 : 12);
      uint32_t prev = 99;
      for (int k = 0; k < nwords; ++k) {
        uint32_t op = rng() % (frame ? 6 : 4);
        if (op == prev) op = (op + 1) % (frame ? 6 : 4);
        uint32_t len = 1 + rng() % (rng() % 4 ? 4 : 90);
        if (op <= 2) {  // the letters must lie inside the source
          if (p < 0 || p >= limit) continue;
          const int64_t room = (limit - 1 - p) / unit + 1;
          if (len > room) len = (uint32_t)room;
        }
        if ((op == 0 || op == 1 || op == 3) && s + len > db.size()) continue;
        if (op >= 4 && len > 2) len = 1 + len % 2;
        for (uint32_t i = 0; i < len; ++i) {
          char ql = '-', sl = '-', ml = ' ';
          uint8_t qc = 0;
          if (op <= 2) {
            qc = frame ? c.plain[si][(size_t)(p % 3) * m + p / 3] : c.plain[si][p];
            ql = Show(qc);
          }
          if (op < 2) {
            const uint8_t sc = db[s];
            const int e = M[(sc & 31) * 32 + (qc & 31)];
            sl = Show(sc);
            w.rescore += e;
            w.positives += e > 0;
            w.identities += op == 0;
            ml = op == 0 ? ql : e > 0 ? '+' : ' ';
          } else if (op == 3) {
            sl = Show(db[s]);
          }
          if (op == 2 || op == 3) {
            ++w.gap_residues;
            w.rescore += i == 0 ? open : ext;
          }
          if (op >= 4) {
            ql = op == 4 ? '\\' : '/';
            ++w.shifts;
            w.rescore += shift;
          }
          if (op <= 2) p += unit;
          if (op == 4) ++p;
          if (op == 5) --p;
          if (op == 0 || op == 1 || op == 3) ++s;
          q.push_back(ql);
          mid.push_back(ml);
          sub.push_back(sl);
        }
        ops.push_back(len << 4 | op);
        ++x.n_runs;
        prev = op;
      }
      w.columns = (uint32_t)q.size();
      w.query_record = c.src[si].first_record;
      if (x.n_runs) {
        const uint32_t cc = frame ? x.q_start / 3 : x.q_start, g = frame ? x.q_start % 3 : 0;
        const uint32_t t = std::min(cc / c.step, c.src[si].tiles - 1);
        w.query_record += g + (c.src[si].tiles > 1 ? c.src[si].stride * t : 0);
      }
      src.push_back(c.src[si]);
      rec.push_back(x);
      want.push_back(q + mid + sub);
      want_rec.push_back(w);
    }
    const uint32_t n = (uint32_t)rec.size();
    size_t used = 0;
    if (GhostmReadRowsHost(c.qseq.data(), nq, c.W, db.data(), (uint32_t)db.size(), M, n, src.data(), rec.data(),
                           ops.data(), ops.size(), c.W, c.step, frame, open, ext, shift, nullptr, nullptr, 0, &used))
      FAIL("round %d: the size call refused: %s", round, g_last.c_str());
    std::vector<uint8_t> rows(used + 8, 0xA7);
    std::vector<GhostmHitReadRows> out(n);
    size_t used2 = 0;
    if (GhostmReadRowsHost(c.qseq.data(), nq, c.W, db.data(), (uint32_t)db.size(), M, n, src.data(), rec.data(),
                           ops.data(), ops.size(), c.W, c.step, frame, open, ext, shift, out.data(), rows.data(), used,
                           &used2))
      FAIL("round %d: refused: %s", round, g_last.c_str());
    if (used2 != used) FAIL("round %d: the two calls disagree on the bytes", round);
    for (size_t k = used; k < rows.size(); ++k)
      if (rows[k] != 0xA7) FAIL("round %d: a byte past the rows was written", round);
    size_t at = 0;
    for (uint32_t h = 0; h < n; ++h, ++trials) {
      const GhostmHitReadRows &g = out[h], &w = want_rec[h];
      if (g.rows_offset != at || g.columns != w.columns || g.identities != w.identities || g.positives != w.positives ||
          g.gap_residues != w.gap_residues || g.rescore != w.rescore || g.shifts != w.shifts || g.pad != 0 ||
          g.query_record != w.query_record)
        FAIL("round %d hit %u: the record differs", round, h);
      if (memcmp(rows.data() + at, want[h].data(), want[h].size()) != 0) FAIL("round %d hit %u: the rows differ", round, h);
      at += want[h].size();
    }
    if (at != used) FAIL("round %d: the bytes do not add up", round);
    // refusals: the canaries stay
    struct Bad {
      const char *reason;
      int what;
    };
    const Bad bads[] = {{"source", 0}, {"ops", 1}, {"word", 2}, {"bounds", 3}, {"rows_cap", 4}, {"null", 5}, {"shift", 6}};
    for (const Bad &b : bads) {
      if (b.what == 6 && !frame) continue;
      std::vector<GhostmBandSource> s2 = src;
      std::vector<GhostmHitPath> r2 = rec;
      std::vector<uint32_t> o2 = ops;
      uint32_t h = 0;
      while (h < n && r2[h].n_runs == 0) ++h;
      if (h == n) break;
      int sh = shift;
      size_t cap = used;
      if (b.what == 0) s2[h].tiles += 1;
      if (b.what == 1) r2[h].ops_offset = ops.size() - r2[h].n_runs + 1;
      if (b.what == 2) o2[r2[h].ops_offset] |= 8u;
      if (b.what == 3) r2[h].q_start = (frame ? 3 : 1) * s2[h].letters;
      if (b.what == 4) cap = used - 1;
      if (b.what == 6) sh = 1;
      std::vector<uint8_t> canary(used + 8, 0xA7);
      std::vector<GhostmHitReadRows> o(n, GhostmHitReadRows{7, 7, 7, 7, 7, 7, 7, 7, 7});
      size_t u = 12345;
      const int code = GhostmReadRowsHost(c.qseq.data(), nq, c.W, db.data(), (uint32_t)db.size(), M, n,
                                          b.what == 5 ? nullptr : s2.data(), r2.data(), o2.data(), o2.size(), c.W, c.step,
                                          frame, open, ext, sh, o.data(), canary.data(), cap, &u);
      if (code == 0 || g_last.find(std::string("GhostmReadRowsHost: ") + b.reason) != 0)
        FAIL("round %d: refusal %s: code %d, %s", round, b.reason, code, g_last.c_str());
      if (u != 12345) FAIL("round %d: refusal %s wrote rows_used", round, b.reason);
      for (uint8_t x : canary)
        if (x != 0xA7) FAIL("round %d: refusal %s wrote rows", round, b.reason);
      for (const GhostmHitReadRows &x : o)
        if (x.columns != 7 || x.shifts != 7) FAIL("round %d: refusal %s wrote a record", round, b.reason);
    }
  }
  printf("%d trials ok\n", trials);
  return 0;
}
