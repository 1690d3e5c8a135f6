// The host model of the adapter stage (ghostm_amd/csrc/read_adapter_host.cpp with
// read_adapter.h), without a device and under the sanitizers: random reads and
// pairs at odd offsets against a second, independent evaluation of the rule on
// the letters themselves (every start's and every fragment length's mismatches
// tabulated first, the answer then found by plain searches over the tables),
// the letters left as they were, and the refusals leaving the records
// untouched.
// Build: g++ -std=c++17 -fsanitize=address,undefined tests/native/test_read_adapter.cpp
//        ghostm_amd/csrc/read_adapter_host.cpp
// Run:   test_read_adapter
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../ghostm_amd/csrc/read_adapter.h"

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

static bool IsBase(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
static char Upper(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 'a' + 'A') : c; }
static char Complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : '?'; }

static bool Matches(char read, char adapter) {
  adapter = Upper(adapter);
  if (adapter == 'N') return true;
  return IsBase(Upper(read)) && Upper(read) == adapter;
}

// adapter_at and the mismatches there, from a table of every start
static void IndependentAdapter(const std::string &read, const std::string &adapter, uint32_t mo, uint32_t err,
                               uint32_t *at, uint32_t *mm_at) {
  const size_t n = read.size(), m = adapter.size();
  std::vector<long> mm(n, -1);  // -1: the start's L is below min_overlap
  for (size_t p = 0; p < n && m; ++p) {
    const size_t L = std::min(m, n - p);
    if (L < mo) continue;
    mm[p] = 0;
    for (size_t i = 0; i < L; ++i) mm[p] += !Matches(read[p + i], adapter[i]);
  }
  *at = (uint32_t)n, *mm_at = 0;
  for (size_t p = n; p-- > 0;) {  // from the back: the last one written is the smallest
    if (mm[p] < 0) continue;
    const size_t L = std::min(m, n - p);
    if ((unsigned long)mm[p] * 100 <= (unsigned long)err * L) *at = (uint32_t)p, *mm_at = (uint32_t)mm[p];
  }
}

static void IndependentPair(const std::string &r1, const std::string &r2, uint32_t po, uint32_t err, uint32_t *len,
                            uint32_t *pm_at, bool *skipped) {
  *len = *pm_at = 0;
  *skipped = po && (r1.size() > 1024 || r2.size() > 1024);
  if (!po || *skipped) return;
  const size_t top = std::min(r1.size(), r2.size());
  for (size_t f = po; f <= top; ++f) {  // upwards: the last one written is the greatest
    // mate 2's first f letters, reverse-complemented, laid beside mate 1's
    std::string rc(f, '?');
    for (size_t i = 0; i < f; ++i) rc[i] = Complement(Upper(r2[f - 1 - i]));
    unsigned long pm = 0;
    for (size_t i = 0; i < f; ++i) pm += !(IsBase(Upper(r1[i])) && Upper(r1[i]) == rc[i]);
    if (pm * 100 <= (unsigned long)err * f) *len = (uint32_t)f, *pm_at = (uint32_t)pm;
  }
}

static std::string RandomAdapter(std::mt19937 &rng, uint32_t m) {
  std::string a(m, 'A');
  for (auto &c : a) c = "ACGTACGTACGTNacgtn"[rng() % 18];
  return a;
}

static void RandomReads() {
  std::mt19937 rng(20261021);
  struct Params {
    uint32_t m1, m2, mo, err, po;
  };
  const Params params[] = {{33, 0, 5, 10, 0}, {1, 0, 1, 0, 0}, {64, 63, 3, 20, 0}, {33, 33, 5, 10, 20},
                           {0, 0, 5, 10, 8},  {0, 13, 5, 0, 1}, {64, 0, 64, 50, 0}, {20, 0, 8, 50, 12}};
  size_t trials = 0, found = 0, pairs_found = 0;
  for (const Params &p : params) {
    const std::string a1 = RandomAdapter(rng, p.m1), a2 = RandomAdapter(rng, p.m2);
    std::vector<uint8_t> letters;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<std::string> reads;
    for (int r = 0; r < 160; ++r) {
      static const uint32_t kFixed[12] = {0, 1, 4, 5, 63, 64, 65, 127, 128, 129, 200, 300};
      uint32_t n = r < 12 ? kFixed[r] : rng() % 260;
      std::string ls(n, 'A');
      for (auto &c : ls) c = "ACGTACGTACGTACGTNacgt#"[rng() % 22];
      if ((r & 1) && p.po && rng() % 3) {  // mate 2 of a read-through pair: a fragment of mate 1, reverse-complemented
        const std::string &m1 = reads.back();
        const size_t f = m1.empty() ? 0 : rng() % std::min<size_t>(m1.size(), n + 1);
        for (size_t i = 0; i < f && i < n; ++i) {
          const char c = Complement(Upper(m1[f - 1 - i]));
          if (c != '?' && rng() % 40) ls[i] = c;
        }
      }
      const std::string &ad = ((r & 1) && p.m2) ? a2 : a1;
      if (n && !ad.empty() && rng() % 3) {  // the adapter from a random start on, a few letters wrong
        const size_t at = rng() % n;
        for (size_t i = 0; i < ad.size() && at + i < n; ++i)
          if (rng() % 25) ls[at + i] = ad[i] == 'N' || ad[i] == 'n' ? 'G' : ad[i];
      }
      const size_t gap = 1 + rng() % 3;  // then one more where needed: every read begins at an odd offset
      letters.insert(letters.end(), gap, ad.empty() ? '#' : (uint8_t)ad[0]);
      if (letters.size() % 2 == 0) letters.push_back('#');
      off.push_back(letters.size());
      len.push_back(n);
      letters.insert(letters.end(), ls.begin(), ls.end());
      reads.push_back(ls);
    }
    letters.push_back('#');
    const std::vector<uint8_t> before = letters;
    std::vector<GhostmAdapterOut> out(off.size());
    CHECK(GhostmAdapterTrimHost(letters.data(), letters.size(), off.data(), len.data(), (uint32_t)off.size(), a1.c_str(),
                                a2.c_str(), p.mo, p.err, p.po, out.data()) == 0);
    CHECK(letters == before);
    for (size_t r = 0; r < off.size(); ++r) {
      uint32_t at, mm, f = 0, pm = 0;
      bool skipped = false;
      IndependentAdapter(reads[r], ((r & 1) && p.m2) ? a2 : a1, p.mo, p.err, &at, &mm);
      if (p.po) IndependentPair(reads[r & ~(size_t)1], reads[r | 1], p.po, p.err, &f, &pm, &skipped);
      const uint32_t n = len[r], kept = std::min(at, f ? f : n);
      CHECK(out[r].adapter_at == at && out[r].adapter_mismatches == mm);
      CHECK(out[r].pair_len == f && out[r].pair_mismatches == pm);
      CHECK(out[r].kept == kept);
      found += at < n;
      pairs_found += f != 0;
      ++trials;
    }
  }
  CHECK(found > 200 && pairs_found > 100);
  std::printf("%zu reads ok, %zu adapters and %zu mates found\n", trials, found, pairs_found);
}

static void LongMates() {
  // 1024 letters are examined, 1025 are not; the sums count the skipped pair once
  std::mt19937 rng(7);
  std::string frag(700, 'A');
  for (auto &c : frag) c = "ACGT"[rng() % 4];
  std::string r1 = frag + std::string(325, 'T'), r2(frag.size(), '?');
  for (size_t i = 0; i < frag.size(); ++i) r2[i] = Complement(frag[frag.size() - 1 - i]);
  r2 += std::string(324, 'T');
  CHECK(r1.size() == 1025 && r2.size() == 1024);
  for (int cut = 0; cut < 2; ++cut) {
    const std::string m1 = r1.substr(0, r1.size() - (size_t)cut);
    const uint8_t *reads[2] = {reinterpret_cast<const uint8_t *>(m1.data()), reinterpret_cast<const uint8_t *>(r2.data())};
    const uint32_t lens[2] = {(uint32_t)m1.size(), (uint32_t)r2.size()};
    AdapterParams p;
    CHECK(MakeAdapterParams("", nullptr, 5, 10, 20, &p).empty() && p.On());
    GhostmAdapterOut out[2];
    AdapterSums sums;
    AdapterTrimReads(reads, lens, 2, p, out, &sums);
    CHECK(out[0].pair_len == (cut ? 700u : 0u) && out[1].pair_len == out[0].pair_len);
    CHECK(sums.pair_skipped == (cut ? 0u : 1u) && sums.pair_found == (cut ? 1u : 0u));
    CHECK(sums.cut_reads == (cut ? 2u : 0u) && sums.cut_letters == (cut ? 324u + 324u : 0u) && sums.emptied == 0);
  }
  std::printf("long mates ok\n");
}

static void Refusals() {
  std::vector<uint8_t> letters(100, 'A');
  uint64_t off[3] = {0, 50, 60};
  uint32_t len[3] = {4, 50, 4};
  const GhostmAdapterOut mark{7, 7, 7, 7, 7};
  GhostmAdapterOut out[3] = {mark, mark, mark};
  auto refused = [&](const char *reason, int rc) {
    CHECK(rc == 1 && g_error.find(std::string("GhostmAdapterTrimHost: ") + reason + ":") == 0);
    CHECK(out[0].kept == 7 && out[1].pair_mismatches == 7 && out[2].adapter_at == 7);
  };
  const uint8_t *l = letters.data();
  refused("param", GhostmAdapterTrimHost(l, 100, off, len, 2, "ACGT", "", 0, 10, 0, out));
  refused("param", GhostmAdapterTrimHost(l, 100, off, len, 2, "ACGT", "", 65, 10, 0, out));
  refused("param", GhostmAdapterTrimHost(l, 100, off, len, 2, "ACGT", "", 5, 51, 0, out));
  refused("param", GhostmAdapterTrimHost(l, 100, off, len, 2, "ACGT", "", 5, 10, 1025, out));
  refused("adapter", GhostmAdapterTrimHost(l, 100, off, len, 2, "ACGU", "", 5, 10, 0, out));
  refused("adapter", GhostmAdapterTrimHost(l, 100, off, len, 2, "ACGT", "AC GT", 5, 10, 0, out));
  refused("adapter", GhostmAdapterTrimHost(l, 100, off, len, 2, std::string(65, 'A').c_str(), "", 5, 10, 0, out));
  CHECK(GhostmAdapterTrimHost(l, 100, off, len, 2, std::string(64, 'n').c_str(), nullptr, 5, 10, 0, out) == 0);
  CHECK(out[0].adapter_at == 4 && out[1].adapter_at == 0 && out[1].kept == 0);  // 64 N's match any 5 letters or more
  out[0] = out[1] = mark;
  refused("null", GhostmAdapterTrimHost(nullptr, 100, off, len, 2, "ACGT", "", 5, 10, 0, out));
  refused("null", GhostmAdapterTrimHost(l, 100, nullptr, len, 2, "ACGT", "", 5, 10, 0, out));
  refused("null", GhostmAdapterTrimHost(l, 100, off, nullptr, 2, "ACGT", "", 5, 10, 0, out));
  refused("null", GhostmAdapterTrimHost(l, 100, off, len, 2, "ACGT", "", 5, 10, 0, nullptr));
  len[1] = 51;
  refused("record", GhostmAdapterTrimHost(l, 100, off, len, 2, "ACGT", "", 5, 10, 0, out));
  len[1] = 50, off[1] = ~0ull;
  refused("record", GhostmAdapterTrimHost(l, 100, off, len, 2, "ACGT", "", 5, 10, 0, out));
  off[1] = 50;
  refused("pairs", GhostmAdapterTrimHost(l, 100, off, len, 3, "ACGT", "", 5, 10, 20, out));
  refused("pairs", GhostmAdapterTrimHost(l, 100, off, len, 1, nullptr, nullptr, 5, 10, 20, out));
  {
    std::vector<uint8_t> big((1u << 24) + 1, 'A');
    uint64_t o1 = 0;
    uint32_t l1 = (1u << 24) + 1;
    refused("length", GhostmAdapterTrimHost(big.data(), big.size(), &o1, &l1, 1, "ACGT", "", 5, 10, 0, out));
  }
  // n == 0 and the off parameters change nothing; off does not read the letters
  CHECK(GhostmAdapterTrimHost(nullptr, 0, nullptr, nullptr, 0, "ACGT", "", 5, 10, 20, nullptr) == 0);
  CHECK(GhostmAdapterTrimHost(l, 100, off, len, 3, "", nullptr, 5, 10, 0, out) == 0);
  CHECK(out[0].kept == 4 && out[1].kept == 50 && out[2].adapter_at == 4 && out[1].pair_len == 0);
  std::printf("refusals ok\n");
}

int main() {
  RandomReads();
  LongMates();
  Refusals();
  std::printf("all ok\n");
  return 0;
}
