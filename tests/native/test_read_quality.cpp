// The host model of the quality stage (ghostm_amd/csrc/read_quality_host.cpp with
// read_quality.h) and the FASTQ reader (fastq_reader.cpp), without a device and
// under the sanitizers: random reads at odd offsets against a second,
// independent O(n^2) evaluation of the rule (every prefix sum recomputed from
// scratch, the stop and the best found by plain searches), the refusals
// leaving letters and records untouched, and the reader on well-formed, CRLF,
// truncated and mismatched files written to a temporary directory.
// Build: g++ -std=c++17 -fsanitize=address,undefined tests/native/test_read_quality.cpp
//        ghostm_amd/csrc/read_quality_host.cpp ghostm_amd/csrc/fastq_reader.cpp
// Run:   test_read_quality <an existing directory to write into>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "../../ghostm_amd/csrc/fastq_reader.h"
#include "../../ghostm_amd/csrc/read_quality.h"

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

// d summed over the first k + 1 walked positions, from scratch
static long SumTo(const std::vector<int> &d, size_t k) {
  long s = 0;
  for (size_t j = 0; j <= k; ++j) s += d[j];
  return s;
}

// the walked index the rule cuts at, or -1: d in walk order
static long CutOf(const std::vector<int> &d) {
  size_t stop = d.size();
  for (size_t k = 0; k < d.size(); ++k)
    if (SumTo(d, k) < 0) {
      stop = k;
      break;
    }
  long best = 0, at = -1;
  for (size_t k = 0; k < stop; ++k) best = std::max(best, SumTo(d, k));
  if (best > 0)
    for (size_t k = 0; k < stop; ++k)
      if (SumTo(d, k) == best) {
        at = (long)k;
        break;
      }
  return at;
}

static GhostmQualOut Independent(std::string *letters, const std::vector<uint8_t> &qual, uint32_t t, uint32_t m,
                                 uint32_t floor) {
  const size_t n = qual.size();
  std::vector<int> q(n), fwd(n), bwd(n);
  GhostmQualOut o{0, 0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    const int b = qual[i];
    o.bad += b < 33 || b > 126;
    q[i] = std::min(std::max(b, 33), 126) - 33;
    fwd[i] = (int)t - q[i];
  }
  for (size_t i = 0; i < n; ++i) bwd[i] = fwd[n - 1 - i];
  const long k3 = CutOf(bwd), k5 = CutOf(fwd);
  const size_t end = k3 < 0 ? n : n - 1 - (size_t)k3, begin = k5 < 0 ? 0 : (size_t)k5 + 1;
  if (end > begin) o.begin = (uint32_t)begin, o.kept = (uint32_t)(end - begin);
  if (o.kept < floor) {
    o.begin = o.kept = 0;
    return o;
  }
  for (size_t i = o.begin; i < (size_t)o.begin + o.kept; ++i)
    if ((uint32_t)q[i] < m) (*letters)[i] = 'N', ++o.masked;
  return o;
}

static void RandomReads() {
  std::mt19937 rng(20261021);
  const uint32_t params[][3] = {{20, 0, 0}, {2, 0, 0}, {20, 10, 30}, {0, 15, 0}, {93, 0, 0}, {30, 93, 5}};
  size_t trials = 0;
  for (const auto &p : params) {
    std::vector<uint8_t> letters, qual;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<std::string> want_letters;
    std::vector<GhostmQualOut> want;
    for (int r = 0; r < 160; ++r) {
      static const uint32_t kFixed[12] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 300, 3};
      const uint32_t n = r < 12 ? kFixed[r] : rng() % 260;
      const size_t gap = 1 + rng() % 3;  // then one more where needed: every read begins at an odd offset
      letters.insert(letters.end(), gap, '#');
      qual.insert(qual.end(), gap, 0xFF);
      if (letters.size() % 2 == 0) letters.push_back('#'), qual.push_back(0xFF);
      off.push_back(letters.size());
      len.push_back(n);
      std::string ls(n, 'A');
      std::vector<uint8_t> qs(n);
      const int kind = (int)(rng() % 4), t = p[0] ? (int)p[0] : 20;
      for (uint32_t i = 0; i < n; ++i) {
        ls[i] = "ACGTN"[rng() % 5];
        const bool low_end = (kind == 1 && i + 20 > n) || (kind == 2 && (i < 5 || i + 30 > n)) || kind == 3;
        int v = low_end ? (int)(rng() % (t + 3)) : t + (int)(rng() % 15) - 2;
        if (rng() % 97 == 0) v = -1 - (int)(rng() % 3);  // a byte below '!'
        if (rng() % 101 == 0) v = 94 + (int)(rng() % 3);  // a byte above '~'
        qs[i] = (uint8_t)(std::min(std::max(v, -33), 200) + 33);
      }
      letters.insert(letters.end(), ls.begin(), ls.end());
      qual.insert(qual.end(), qs.begin(), qs.end());
      want.push_back(Independent(&ls, qs, p[0], p[1], p[2]));
      want_letters.push_back(ls);
    }
    letters.push_back('#');
    qual.push_back(0xFF);
    std::vector<GhostmQualOut> out(off.size());
    CHECK(GhostmQualityTrimHost(letters.data(), qual.data(), letters.size(), off.data(), len.data(), (uint32_t)off.size(),
                                p[0], p[1], p[2], out.data()) == 0);
    std::vector<uint8_t> inside(letters.size(), 0);
    for (size_t r = 0; r < off.size(); ++r) {
      CHECK(out[r].begin == want[r].begin && out[r].kept == want[r].kept);
      CHECK(out[r].masked == want[r].masked && out[r].bad == want[r].bad);
      CHECK(std::equal(want_letters[r].begin(), want_letters[r].end(), letters.begin() + (long)off[r]));
      std::fill(inside.begin() + (long)off[r], inside.begin() + (long)(off[r] + len[r]), 1);
      ++trials;
    }
    for (size_t i = 0; i < letters.size(); ++i) CHECK(inside[i] || letters[i] == '#');
  }
  std::printf("%zu reads ok\n", trials);
}

static void Refusals() {
  std::vector<uint8_t> letters(100, 'A'), qual(100, 'I');
  const std::vector<uint8_t> before = letters;
  uint64_t off[2] = {0, 50};
  uint32_t len[2] = {4, 50};
  GhostmQualOut out[2] = {{7, 7, 7, 7}, {7, 7, 7, 7}};
  auto refused = [&](const char *reason, int rc) {
    CHECK(rc == 1 && g_error.find(std::string("GhostmQualityTrimHost: ") + reason + ":") == 0);
    CHECK(letters == before && out[0].begin == 7 && out[1].bad == 7);
  };
  refused("param", GhostmQualityTrimHost(letters.data(), qual.data(), 100, off, len, 2, 94, 0, 0, out));
  refused("param", GhostmQualityTrimHost(letters.data(), qual.data(), 100, off, len, 2, 0, 94, 0, out));
  refused("param", GhostmQualityTrimHost(letters.data(), qual.data(), 100, off, len, 2, 0, 0, (1u << 24) + 1, out));
  refused("null", GhostmQualityTrimHost(nullptr, qual.data(), 100, off, len, 2, 20, 0, 0, out));
  refused("null", GhostmQualityTrimHost(letters.data(), qual.data(), 100, nullptr, len, 2, 20, 0, 0, out));
  refused("null", GhostmQualityTrimHost(letters.data(), qual.data(), 100, off, len, 2, 20, 0, 0, nullptr));
  len[1] = 51;
  refused("record", GhostmQualityTrimHost(letters.data(), qual.data(), 100, off, len, 2, 20, 0, 0, out));
  len[1] = 50, off[1] = ~0ull;
  refused("record", GhostmQualityTrimHost(letters.data(), qual.data(), 100, off, len, 2, 20, 0, 0, out));
  off[1] = 50;
  {
    std::vector<uint8_t> big((1u << 24) + 1, 'A');
    uint64_t o1 = 0;
    uint32_t l1 = (1u << 24) + 1;
    CHECK(GhostmQualityTrimHost(big.data(), big.data(), big.size(), &o1, &l1, 1, 20, 0, 0, out) == 1);
    CHECK(g_error.find("GhostmQualityTrimHost: length:") == 0 && out[0].begin == 7);
  }
  // n == 0 and the off parameters change nothing; off does not read the qualities
  CHECK(GhostmQualityTrimHost(nullptr, nullptr, 0, nullptr, nullptr, 0, 20, 0, 0, nullptr) == 0);
  CHECK(GhostmQualityTrimHost(letters.data(), nullptr, 0, off, len, 0, 20, 0, 0, out) == 0);
  std::fill(qual.begin(), qual.end(), 0);
  CHECK(GhostmQualityTrimHost(letters.data(), qual.data(), 100, off, len, 2, 0, 0, 0, out) == 0);
  CHECK(letters == before && out[0].kept == 4 && out[1].kept == 50 && out[0].bad == 0 && out[1].begin == 0);
  std::printf("refusals ok\n");
}

static std::string WriteFile(const std::string &dir, const char *name, const std::string &text) {
  const std::string path = dir + "/" + name;
  std::ofstream f(path.c_str(), std::ios::binary);
  f << text;
  return path;
}

static std::string ErrorOf(const std::string &path) {
  try {
    FastqSet set;
    ReadFastqSet(path, &set);
  } catch (FastqError &e) {
    return e.what();
  }
  return "";
}

static void Reader(const std::string &dir) {
  const std::string good = "@r1 first\nACGT\n+\nIIII\n\n@  r2\nAC\n+r2 again\n!~\n@e\n\n+\n\n\n\n";
  for (int crlf = 0; crlf < 2; ++crlf) {
    std::string text = good;
    if (crlf) {
      text.clear();
      for (char c : good) text += c == '\n' ? std::string("\r\n") : std::string(1, c);
    }
    FastqSet set;
    ReadFastqSet(WriteFile(dir, crlf ? "crlf.fq" : "good.fq", text), &set);
    CHECK(set.names.size() == 3 && set.names[0] == "r1 first" && set.names[1] == "r2" && set.names[2] == "e");
    CHECK(set.letters == "ACGTAC" && set.qual == "IIII!~");
    CHECK(set.off[0] == 0 && set.off[1] == 4 && set.off[2] == 6 && set.len[0] == 4 && set.len[1] == 2 && set.len[2] == 0);
    CHECK(LooksLikeFastq(dir + (crlf ? "/crlf.fq" : "/good.fq")));
  }
  {  // a last line without its newline; a quality line that begins with '@' or '>' is no header
    FastqSet set;
    ReadFastqSet(WriteFile(dir, "noeol.fq", "@a\nACG\n+\n@>I\n@b\nA\n+\n>"), &set);
    CHECK(set.names.size() == 2 && set.qual == "@>I>" && set.letters == "ACGA");
  }
  CHECK(ErrorOf(WriteFile(dir, "empty.fq", "")) == "");
  CHECK(ErrorOf(WriteFile(dir, "t1.fq", "@a\nACGT\n+\nIIII\n@b\nAC\n")) == "fastq: record 2: truncated");
  CHECK(ErrorOf(WriteFile(dir, "t2.fq", "@a\nACGT\n+\n")) == "fastq: record 1: truncated");
  CHECK(ErrorOf(WriteFile(dir, "t3.fq", "@a\n")) == "fastq: record 1: truncated");
  CHECK(ErrorOf(WriteFile(dir, "mm.fq", "@a\nACGT\n+\nIII\n")) == "fastq: record 1: 4 letters, 3 qualities");
  CHECK(ErrorOf(WriteFile(dir, "plus.fq", "@a\nACGT\nIIII\n+\n")) == "fastq: record 1: no '+' line");
  CHECK(ErrorOf(WriteFile(dir, "multi.fq", "@a\nACGT\nACGT\n+\nIIIIIIII\n")) == "fastq: record 1: no '+' line");
  CHECK(ErrorOf(WriteFile(dir, "blank.fq", "@a\nACGT\n\n+\nIIII\n")) == "fastq: record 1: no '+' line");
  CHECK(ErrorOf(WriteFile(dir, "fa.fq", "@a\nACGT\n+\nIIII\n>b\nACGT\n")) == "fastq: record 2: header does not begin with '@'");
  CHECK(ErrorOf(dir + "/none.fq") == "fastq: cannot open " + dir + "/none.fq");
  CHECK(!LooksLikeFastq(WriteFile(dir, "x.fa", ">a\nACGT\n")) && !LooksLikeFastq(dir + "/none.fq"));
  std::printf("reader ok\n");
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::printf("usage: test_read_quality DIR\n");
    return 2;
  }
  RandomReads();
  Refusals();
  Reader(argv[1]);
  std::printf("all ok\n");
  return 0;
}
