// The host model of the low-complexity mask (ghostm_amd/csrc/query_mask_host.cpp
// with query_mask.h), without a device and under the sanitizers: random sources
// through random tile layouts against a second, independent evaluation (counts
// by sorting, runs by reaching out from every trigger), two runs of more than
// 128 low windows whose only trigger is the first window, and the last, the
// table of window 12, the flag-word plan, and the refusals leaving the records
// untouched.
// Build: g++ -std=c++17 -fsanitize=address,undefined tests/native/test_query_mask.cpp
//        ghostm_amd/csrc/query_mask_host.cpp
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../ghostm_amd/csrc/query_mask.h"

namespace ghostm {
static std::string g_error;
void SetLastErrorMessage(const std::string &m) { g_error = m; }
}  // namespace ghostm

using namespace ghostm;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

// low / trigger of every window: the counts from the sorted window, the entropy term in floating point first to
// see that the integer rule is SEG's (within the table's rounding), then the integer rule itself
static void Flags(const std::vector<uint8_t> &s, uint32_t w, uint32_t k1, uint32_t k2, std::vector<char> *low,
                  std::vector<char> *trig) {
  const size_t nw = s.size() >= w ? s.size() - w + 1 : 0;
  low->assign(nw, 0);
  trig->assign(nw, 0);
  for (size_t i = 0; i < nw; ++i) {
    std::vector<uint8_t> win(s.begin() + i, s.begin() + i + w);
    std::sort(win.begin(), win.end());
    if (win.back() >= 23) continue;
    int64_t sum = 0;
    double bits = 0;
    for (size_t a = 0; a < win.size();) {
      size_t b = a;
      while (b < win.size() && win[b] == win[a]) ++b;
      const double c = (double)(b - a);
      sum += std::lround(1024.0 * c * std::log2(c));
      bits -= c / w * std::log2(c / w);
      a = b;
    }
    const int64_t d = 100 * (std::lround(1024.0 * w * std::log2((double)w)) - sum);
    CHECK(std::fabs(d / (102400.0 * w) - bits) < 0.01);  // d is the window's entropy in hundredths of a bit x 1024 w
    (*low)[i] = d <= (int64_t)k2 * 1024 * w;
    (*trig)[i] = d <= (int64_t)k1 * 1024 * w;
  }
}

// masked letters: from every trigger out over the low windows on both sides
static std::vector<char> Masked(const std::vector<uint8_t> &s, uint32_t w, uint32_t k1, uint32_t k2) {
  std::vector<char> low, trig, mask(s.size(), 0);
  Flags(s, w, k1, k2, &low, &trig);
  for (size_t t = 0; t < trig.size(); ++t) {
    if (!trig[t]) continue;
    CHECK(low[t]);
    size_t a = t, b = t;
    while (a > 0 && low[a - 1]) --a;
    while (b + 1 < low.size() && low[b + 1]) ++b;
    std::fill(mask.begin() + a, mask.begin() + b + w, 1);
  }
  return mask;
}

struct Set {
  std::vector<uint8_t> rec;
  std::vector<GhostmBandSource> src;
  std::vector<std::vector<uint8_t>> letters;
  uint32_t W, step;
};

// the sources' letters laid out as tile records, `per` sources of one length interleaved (stride per)
static Set LayOut(const std::vector<std::vector<uint8_t>> &letters, uint32_t W, uint32_t step, uint32_t per) {
  Set s;
  s.W = W;
  s.step = step;
  s.letters = letters;
  uint32_t rows = 0;
  for (size_t b = 0; b < letters.size(); b += per) {
    const uint32_t m = (uint32_t)letters[b].size(), tiles = TileCount(m, W, step);
    for (uint32_t f = 0; f < per; ++f) {
      CHECK(letters[b + f].size() == m);
      s.src.push_back(GhostmBandSource{rows + f, per, tiles, m});
    }
    s.rec.resize((size_t)(rows + tiles * per) * W, 23);
    for (uint32_t t = 0; t < tiles; ++t)
      for (uint32_t f = 0; f < per; ++f) {
        const uint32_t st = TileStart(t, tiles, m, W, step);
        for (uint32_t k = 0; k < W && st + k < m; ++k) s.rec[(size_t)(rows + t * per + f) * W + k] = letters[b + f][st + k];
      }
    rows += tiles * per;
  }
  return s;
}

static void RunAndCheck(const Set &s, uint32_t w, uint32_t k1, uint32_t k2) {
  std::vector<uint8_t> got = s.rec, want = s.rec;
  const uint32_t nq = (uint32_t)(s.rec.size() / s.W);
  std::vector<uint32_t> masked(nq, 99), count(nq, 0);
  CHECK(GhostmMaskRecordsHost(got.data(), nq, s.W, (uint32_t)s.src.size(), s.src.data(), s.step, w, k1, k2,
                              masked.data()) == 0);
  for (size_t h = 0; h < s.src.size(); ++h) {
    const GhostmBandSource &S = s.src[h];
    if (S.letters < w) continue;
    const std::vector<char> mask = Masked(s.letters[h], w, k1, k2);
    for (uint32_t t = 0; t < S.tiles; ++t) {
      const uint32_t st = TileStart(t, S.tiles, S.letters, s.W, s.step), rec = S.first_record + (S.tiles > 1 ? S.stride * t : 0);
      for (uint32_t k = 0; k < s.W && st + k < S.letters; ++k)
        if (mask[st + k]) {
          want[(size_t)rec * s.W + k] = 23;
          ++count[rec];
        }
    }
  }
  CHECK(got == want);
  CHECK(masked == count);
}

int main() {
  std::mt19937 rng(12345);
  auto pick = [&](uint32_t n) { return (uint32_t)(rng() % n); };
  const MaskTable tab = MakeMaskTable();
  const uint32_t t12[13] = {0, 0, 2048, 4869, 8192, 11888, 15882, 20123, 24576, 29214, 34017, 38967, 44052};
  for (int c = 0; c <= 12; ++c) CHECK(tab.T[c] == t12[c]);
  CHECK(tab.T[32] == 32 * 5 * 1024);

  // random sources, planted stretches, X and '*'
  const uint32_t levels[4][2] = {{220, 250}, {0, 0}, {250, 250}, {0, 500}};
  const uint32_t layouts[5][3] = {{20, 7, 1}, {64, 64, 6}, {127, 64, 1}, {127, 1, 6}, {33, 5, 6}};
  int trials = 0, some = 0;
  for (uint32_t w : {6u, 12u, 32u})
    for (const auto &lv : levels)
      for (const auto &lay : layouts) {
        std::vector<std::vector<uint8_t>> letters;
        for (uint32_t m : {w - 1, w, w + 1, 63u, 64u, 65u, 63 + w, 64 + w - 1, 64 + w, 200u, 300u})
          for (uint32_t f = 0; f < 6; ++f) {
            std::vector<uint8_t> s(m);
            for (auto &c : s) c = (uint8_t)pick(f % 2 ? 20 : 23);
            for (uint32_t k = pick(3); k > 0 && m >= w; --k) {  // a stretch drawn from 1 to 6 letters
              const uint32_t n = std::min(m, w + pick(2 * w)), at = pick(m - n + 1), pool = 1 + pick(6), base = pick(17);
              for (uint32_t p = 0; p < n; ++p) s[at + p] = (uint8_t)(base + pick(pool));
            }
            if (f >= 4)
              for (uint32_t k = 0; k < 1 + m / 40; ++k) s[pick(m)] = (uint8_t)(23 + pick(2));
            letters.push_back(s);
          }
        const Set set = LayOut(letters, lay[0], lay[1], lay[2]);
        RunAndCheck(set, w, lv[0], lv[1]);
        for (const auto &s : letters) {
          const std::vector<char> mk = Masked(s, w, lv[0], lv[1]);
          some += std::count(mk.begin(), mk.end(), 1) > 0;
        }
        trials += (int)letters.size();
      }
  CHECK(some > trials / 10 && some < trials - trials / 10);

  // more than 128 low windows in a row, the only trigger the first window: ABCD x 3 (2.0 bits), then EABCD
  // repeated (every later window holds five letters, at least 2.23 bits); and its mirror, the only trigger the last
  {
    const uint32_t w = 12;
    std::vector<uint8_t> s;
    for (int p = 0; p < 12; ++p) s.push_back((uint8_t)(p % 4));
    for (int p = 0; p < 200; ++p) s.push_back((uint8_t)("\4\0\1\2\3"[p % 5]));
    for (int p = 0; p < 17; ++p) s.push_back((uint8_t)(6 + p));  // seventeen distinct letters close the run
    for (int mirror = 0; mirror < 2; ++mirror) {
      std::vector<char> low, trig;
      Flags(s, w, 220, 250, &low, &trig);
      const size_t first = mirror ? low.size() - 1 : 0;
      size_t run = 0;
      for (size_t i = first; i < low.size() && low[i]; mirror ? --i : ++i) ++run;
      CHECK(run > 128 && trig[first] && std::count(trig.begin(), trig.end(), 1) == 1);
      for (const auto &lay : layouts) {
        std::vector<std::vector<uint8_t>> six(6, s);
        RunAndCheck(LayOut(six, lay[0], lay[1], lay[2]), w, 220, 250);
      }
      const std::vector<char> mk = Masked(s, w, 220, 250);
      CHECK((size_t)std::count(mk.begin(), mk.end(), 1) == run + w - 1);
      std::reverse(s.begin(), s.end());
    }
  }

  // the flag-word plan
  {
    const GhostmBandSource src[4] = {{0, 1, 1, 11}, {1, 1, 1, 12}, {2, 1, 1, 75}, {3, 1, 2, 76 + 64}};
    const MaskPlan p = PlanMask(4, src, 12);
    CHECK(p.word_off[0] == 0 && p.word_off[1] == 0 && p.word_off[2] == 1 && p.word_off[3] == 2 && p.word_off[4] == 5);
    CHECK(p.windows == 1 + 64 + 129 && p.sources == 3);
  }

  // refusals: the reason, the records and masked[] untouched
  {
    std::vector<uint8_t> rec(4 * 20, 5), before = rec;
    std::vector<uint32_t> masked(4, 77);
    struct Bad {
      const char *reason;
      std::vector<GhostmBandSource> src;
      uint32_t step, w, k1, k2;
    };
    const std::vector<GhostmBandSource> ok{{0, 1, 3, 30}};
    const std::vector<Bad> bad = {
        {"window:", ok, 5, 5, 220, 250},   {"window:", ok, 5, 33, 220, 250},  {"levels:", ok, 5, 12, 251, 250},
        {"levels:", ok, 5, 12, 0, 501},    {"source:", ok, 0, 12, 220, 250},  {"source:", ok, 21, 12, 220, 250},
        {"source:", {{0, 1, 0, 30}}, 5, 12, 220, 250}, {"source:", {{0, 1, 1, 0}}, 5, 12, 220, 250},
        {"source:", {{0, 1, 2, 30}}, 5, 12, 220, 250}, {"source:", {{0, 0, 3, 30}}, 5, 12, 220, 250},
        {"source:", {{2, 1, 3, 30}}, 5, 12, 220, 250}, {"overlap:", {{0, 1, 3, 30}, {2, 1, 1, 20}}, 5, 12, 220, 250},
    };
    for (const Bad &b : bad) {
      g_error.clear();
      CHECK(GhostmMaskRecordsHost(rec.data(), 4, 20, (uint32_t)b.src.size(), b.src.data(), b.step, b.w, b.k1, b.k2,
                                  masked.data()) != 0);
      CHECK(g_error.find(b.reason) != std::string::npos);
      CHECK(rec == before && masked == std::vector<uint32_t>(4, 77));
    }
    CHECK(GhostmMaskRecordsHost(nullptr, 4, 20, 1, ok.data(), 5, 12, 220, 250, masked.data()) != 0);
    CHECK(g_error.find("null:") != std::string::npos);
    CHECK(GhostmMaskRecordsHost(rec.data(), 4, 20, 1, ok.data(), 5, 12, 220, 250, masked.data()) == 0);
    CHECK(rec[0] == 23 && rec[2 * 20 + 19] == 23 && rec[3 * 20] == 5);
    CHECK(masked[0] == 20 && masked[1] == 20 && masked[2] == 20 && masked[3] == 0);
  }
  std::printf("%d trials ok\n", trials);
  return 0;
}
