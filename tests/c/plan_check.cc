// plan_check.cc -- the batch planner (sproxy_amd/csrc/md5_plan.cc) on its
// own: no device, no HIP runtime.  The planner's one way to the device,
// md5hip_cu_count(), is defined here and driven by g_cus, so every threshold
// is checked where it lies for 8, 256 and 304 compute units.
// tests/test_plan_host.py builds this with the planner under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../sproxy_amd/csrc/md5_internal.h"

static int g_cus = 256;
extern "C" int md5hip_cu_count(void) { return g_cus; }

static int g_checks = 0;
#define CHECK(c)                                                                       \
  do {                                                                                 \
    ++g_checks;                                                                        \
    if (!(c)) {                                                                        \
      fprintf(stderr, "%s:%d: (cus %d) failed: %s\n", __FILE__, __LINE__, g_cus, #c);  \
      exit(1);                                                                         \
    }                                                                                  \
  } while (0)

typedef std::vector<uint32_t> Lens;

static uint32_t key_of(uint32_t len) { return (len >> 6) + 1; }

// the contract, naively: by key descending, ties in index order
static std::vector<uint32_t> naive_order(const Lens& lens) {
  std::vector<uint32_t> o(lens.size());
  for (size_t i = 0; i < o.size(); ++i) o[i] = (uint32_t)i;
  std::stable_sort(o.begin(), o.end(),
                   [&](uint32_t a, uint32_t b) { return key_of(lens[a]) > key_of(lens[b]); });
  return o;
}

static void check_order(const Lens& lens) {
  std::vector<uint32_t> got(lens.size() + 1, 0xdeadbeefu);      // one past: must stay untouched
  CHECK(md5hip_plan_order(lens.data(), lens.size(), got.data()) == 0);
  CHECK(got[lens.size()] == 0xdeadbeefu);
  got.pop_back();
  CHECK(got == naive_order(lens));
}

static uint32_t g_rng = 12345;
static uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u, g_rng >> 8; }

static void order_small() {
  for (uint32_t n : {0u, 1u, 63u, 64u, 65u}) {
    Lens mixed(n), equal(n, 16384), low_bits(n);
    for (uint32_t i = 0; i < n; ++i) {
      mixed[i] = rnd() % 70000;
      low_bits[i] = 4096 + (63 - i % 64);          // differ only below bit 6: all ties
    }
    check_order(mixed);
    check_order(equal);
    check_order(low_bits);
    std::vector<uint32_t> o(n + 1);
    CHECK(md5hip_plan_order(low_bits.data(), n, o.data()) == 0);
    for (uint32_t i = 0; i < n; ++i) CHECK(o[i] == i);
  }
  uint32_t one = 5, out = 0;
  CHECK(md5hip_plan_order(nullptr, 0, nullptr) == 0);
  CHECK(md5hip_plan_order(nullptr, 1, &out) == -EINVAL);
  CHECK(md5hip_plan_order(&one, 1, nullptr) == -EINVAL);
  CHECK(md5hip_plan_order(&one, 0x100000000ull, &out) == -EINVAL);
}

// n >= 2 * 2^17 splits the index range over helper threads
static void order_threaded() {
  const uint32_t classes[5] = {0, 100, 4096, 16384, 70000};
  for (uint32_t n : {(1u << 18) - 1, 1u << 18, (1u << 18) + 1}) {
    Lens lens(n);
    for (uint32_t i = 0; i < n; ++i) lens[i] = classes[rnd() % 5];
    check_order(lens);
  }
}

// a key past 2^20: the comparison sort
static void order_fallback() {
  check_order(Lens{100, 0xffffffffu, 64, 0xffffffffu, 63});
  Lens lens(1000);
  for (uint32_t i = 0; i < 1000; ++i) lens[i] = i % 97 == 5 ? 0xffffffffu - (i & 64) : rnd() % 5000;
  check_order(lens);
}

// md5hip_plan_desc's variant, checked against the histogram's: the same
// choice, and bucket starts where each key begins in the longest-first order
static int plan_both(const Lens& lens) {
  const uint64_t n = lens.size();
  std::vector<uint32_t> order(n);
  const int v = md5hip_plan_desc(lens.data(), n, order.data());
  CHECK(order == naive_order(lens));
  uint32_t kmax = 1;
  for (uint32_t L : lens) kmax = std::max(kmax, key_of(L));
  CHECK(kmax <= MD5HIP_HIST_KMAX);
  std::vector<uint32_t> hist(kmax + 1, 0), start(kmax + 1, 0xdeadbeefu);
  for (uint32_t L : lens) hist[key_of(L)]++;
  CHECK(md5hip_plan_hist(hist.data(), kmax, n, start.data()) == v);
  CHECK(md5hip_plan_hist(hist.data(), kmax, n, nullptr) == v);
  uint64_t r = 0;
  for (uint32_t k = kmax; k >= 1; --k) {
    CHECK(start[kmax - k] == r);
    if (hist[k]) CHECK(key_of(lens[order[r]]) == k && (r == 0 || key_of(lens[order[r - 1]]) > k));
    r += hist[k];
  }
  CHECK(start[kmax] == n);
  return v;
}

// C3's classes, 4 KiB << 0..8, one chunk in 8 a ragged tail
static Lens c3_like(uint32_t n, uint32_t times) {
  Lens lens;
  for (uint32_t t = 0; t < times; ++t)
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t c = 4096u << (rnd() % 9);
      lens.push_back(rnd() % 8 == 0 ? 1 + rnd() % (c - 1) : c);
    }
  return lens;
}

// a few long chunks among thousands of 16 KiB ones; 8 MiB - 64 B has the
// largest key a histogram holds (MD5HIP_HIST_KMAX)
static Lens few_long(uint32_t times) {
  Lens lens;
  for (uint32_t t = 0; t < times; ++t) {
    for (uint32_t i = 0; i < 48000; ++i) lens.push_back(16384);
    for (uint32_t i = 0; i < 8; ++i) lens[lens.size() - 1 - 5000 * i] = (8u << 20) - 64;
  }
  return lens;
}

static void plan_thresholds() {
  const uint32_t c = (uint32_t)g_cus;
  // two groups per CU: lane-direct up to it, XDMA past it (16 KiB < HYBRID's 256 KiB)
  CHECK(plan_both(Lens(2 * c * 64 - 1, 16384)) == MD5HIP_DESC_LANE);
  CHECK(plan_both(Lens(2 * c * 64, 16384)) == MD5HIP_DESC_LANE);
  CHECK(plan_both(Lens(2 * c * 64 + 1, 16384)) == MD5HIP_DESC_XDMA);
  // one group per CU: fed pairs up to it, when a chunk has two whole blocks
  for (uint32_t len : {64u, 127u}) {                               // bmax 1
    CHECK(plan_both(Lens(c * 64 - 1, len)) == MD5HIP_DESC_LANE);
    CHECK(plan_both(Lens(c * 64, len)) == MD5HIP_DESC_LANE);
    CHECK(plan_both(Lens(c * 64 + 1, len)) == MD5HIP_DESC_LANE);
  }
  CHECK(MD5HIP_FED_MIN_BLOCKS == 2);
  CHECK(plan_both(Lens(c * 64 - 1, 128)) == MD5HIP_DESC_FED);      // bmax 2
  CHECK(plan_both(Lens(c * 64, 128)) == MD5HIP_DESC_FED);
  CHECK(plan_both(Lens(c * 64 + 1, 128)) == MD5HIP_DESC_LANE);
  Lens one_long(c * 64, 100);
  one_long.back() = 128;                                           // one chunk is enough
  CHECK(plan_both(one_long) == MD5HIP_DESC_FED);
  CHECK(md5hip_fed_fits(c) && !md5hip_fed_fits((uint64_t)c + 1) && md5hip_fed_fits(0));
  // HYBRID's 256 KiB: a long chunk just under it keeps XDMA whatever the rest
  Lens under(2 * c * 64 + 1, 4096);
  under[7] = MD5HIP_HYBRID_LONG_BLOCKS * 64 - 1;
  CHECK(plan_both(under) == MD5HIP_DESC_XDMA);
  under[7] = MD5HIP_HYBRID_LONG_BLOCKS * 64;
  CHECK(plan_both(under) == MD5HIP_DESC_HYBRID);
  // mixed batches: the choice is the same from the order and from the
  // histogram at every CU count; at 256 CUs one C3 batch is chain-bound
  // (HYBRID) and three coalesced hold enough work for BALANCED
  const int one = plan_both(c3_like(72000, 1)), three = plan_both(c3_like(72000, 3));
  const int few = plan_both(few_long(1)), few3 = plan_both(few_long(3));
  if (c == 256) {
    CHECK(one == MD5HIP_DESC_HYBRID && three == MD5HIP_DESC_BALANCED);
    CHECK(few == MD5HIP_DESC_HYBRID && few3 == MD5HIP_DESC_HYBRID);     // one group of long firsts: little work
  }
  if (c == 8) CHECK(one == MD5HIP_DESC_BALANCED);                        // the same work on 32 SIMDs
  // equal long chunks do not stand out
  CHECK(plan_both(Lens(2 * c * 64 + 1, 1u << 20)) == MD5HIP_DESC_XDMA);
}

static void plan_edges() {
  uint32_t hist[4] = {0, 3, 0, 1}, start[4] = {9, 9, 9, 9}, order[4];
  CHECK(md5hip_plan_desc(nullptr, 0, nullptr) == MD5HIP_DESC_XDMA);
  CHECK(md5hip_plan_desc(nullptr, 1, order) == -EINVAL);
  CHECK(md5hip_plan_hist(nullptr, 3, 4, start) == -EINVAL);
  CHECK(md5hip_plan_hist(hist, MD5HIP_HIST_KMAX + 1, 4, start) == -EINVAL);
  CHECK(start[0] == 9);                                            // refused before anything is written
  CHECK(md5hip_plan_hist(hist, 0, 4, start) == MD5HIP_DESC_XDMA);  // no keys: the end only
  CHECK(start[0] == 0 && start[1] == 9);
  CHECK(md5hip_plan_hist(hist, 3, 0, start) == MD5HIP_DESC_XDMA);  // n == 0: starts still filled
  CHECK(start[0] == 0 && start[1] == 1 && start[2] == 1 && start[3] == 4);
  uint32_t none[4] = {0, 0, 0, 0};
  CHECK(md5hip_plan_hist(none, 3, 4, start) == MD5HIP_DESC_XDMA);  // an empty histogram
  CHECK(start[0] == 0 && start[3] == 0);
  // 8 MiB is past the histogram's keys; the order still plans it
  const uint32_t kbig = key_of(8u << 20);
  std::vector<uint32_t> big(kbig + 1, 0);
  CHECK(kbig == MD5HIP_HIST_KMAX + 1 && md5hip_plan_hist(big.data(), kbig, 1, nullptr) == -EINVAL);
  Lens lens = few_long(1);
  lens[0] = 8u << 20;
  std::vector<uint32_t> o(lens.size());
  CHECK(md5hip_plan_desc(lens.data(), lens.size(), o.data()) == MD5HIP_DESC_HYBRID && o[0] == 0);
}

static void lines() {
  for (uint64_t bytes : {1000ull, 1ull << 40}) {
    CHECK(md5hip_lines_choice(MD5HIP_DESC_XDMA, bytes / 2, bytes) == MD5HIP_DESC_XDMA);
    CHECK(md5hip_lines_choice(MD5HIP_DESC_XDMA, bytes / 2 + 1, bytes) == MD5HIP_DESC_LINES);
    CHECK(md5hip_lines_choice(MD5HIP_DESC_HYBRID, bytes, bytes) == MD5HIP_DESC_HYBRID);
  }
  CHECK(md5hip_lines_choice(MD5HIP_DESC_XDMA, 0, 0) == MD5HIP_DESC_XDMA);
  // through md5hip_plan_desc_at: a batch past the small ones (XDMA), chunks
  // 16-B but not 128-B aligned
  const uint64_t n = 2 * (uint64_t)g_cus * 64 + 2;
  Lens lens(n, 1024);
  std::vector<uint64_t> addrs(n);
  std::vector<uint32_t> order(n);
  for (uint64_t i = 0; i < n; ++i) addrs[i] = 0x1000 + i * 1024 + (i < n / 2 ? 16 : 0);
  CHECK(md5hip_plan_desc_at(lens.data(), addrs.data(), n, order.data()) == MD5HIP_DESC_XDMA);   // half
  addrs[n - 1] += 48;
  CHECK(md5hip_plan_desc_at(lens.data(), addrs.data(), n, order.data()) == MD5HIP_DESC_LINES);  // past half
  addrs[n - 1] += 1;                                                // not 16-B aligned: not counted
  CHECK(md5hip_plan_desc_at(lens.data(), addrs.data(), n, order.data()) == MD5HIP_DESC_XDMA);
  CHECK(md5hip_plan_desc_at(lens.data(), nullptr, n, order.data()) == -EINVAL);
  CHECK(md5hip_plan_desc_at(nullptr, nullptr, 0, nullptr) == MD5HIP_DESC_XDMA);
}

static void crc_choice() {
  const uint64_t c = (uint64_t)g_cus;
  for (uint64_t mean : {0ull, 1ull, 2047ull}) {                     // short chunks: 12 per CU
    CHECK(md5hip_crc_desc_choice(12 * c - 1, mean) == CRC32HIP_SPLIT);
    CHECK(md5hip_crc_desc_choice(12 * c, mean) == CRC32HIP_SPLIT);
    CHECK(md5hip_crc_desc_choice(12 * c + 1, mean) == CRC32HIP_XDMA16);
    CHECK(md5hip_crc_desc_choice(128 * c, mean) == CRC32HIP_XDMA16);
  }
  for (uint64_t mean : {2048ull, 1ull << 20}) {                     // from 2 KiB: 128 per CU
    CHECK(md5hip_crc_desc_choice(12 * c + 1, mean) == CRC32HIP_SPLIT);
    CHECK(md5hip_crc_desc_choice(128 * c - 1, mean) == CRC32HIP_SPLIT);
    CHECK(md5hip_crc_desc_choice(128 * c, mean) == CRC32HIP_SPLIT);
    CHECK(md5hip_crc_desc_choice(128 * c + 1, mean) == CRC32HIP_XDMA16);
  }
  // the launchers' entry: length 0 = not known, 16 per CU
  CHECK(md5hip_crc_split_fits(16 * c, 0) && !md5hip_crc_split_fits(16 * c + 1, 0));
  CHECK(md5hip_crc_split_fits(12 * c, 2047) && !md5hip_crc_split_fits(12 * c + 1, 2047));
  CHECK(md5hip_crc_split_fits(128 * c, 2048) && !md5hip_crc_split_fits(128 * c + 1, 2048));
}

int main() {
  order_small();
  order_threaded();
  order_fallback();
  for (int cus : {256, 8, 304}) {
    g_cus = cus;
    plan_thresholds();
    plan_edges();
    lines();
    crc_choice();
  }
  printf("plan ok: %d checks at 256, 8 and 304 CUs\n", g_checks);
  return 0;
}
