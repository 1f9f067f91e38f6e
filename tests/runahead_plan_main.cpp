// Host program behind tests/test_runahead_plan.py: the touch plan of csrc/runahead.h, exhaustively, on the CPU.
//   for every range size x issuing workgroups x slots:  every offset lies in the range with its whole dword, no line is touched twice, and when the
//   slots cover the range every line (that holds a whole dword) is touched exactly once; otherwise a prefix.
// Every planned dword is also READ from a heap buffer of exactly the range's size, so a build with -fsanitize=address,undefined turns an offset past
// the range into an error rather than a number.  The device half's decomposition (wave-uniform first line of a slot + lane) is replayed against
// ra_offset, and the descriptor-to-argument step (ra_make) is run on the chain's ranges and on the refused forms.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "runahead.h"

using namespace mode;

static int fails = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (fails++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                      \
  } while (0)

static unsigned long run_case(long bytes, int nwg, int slots) {
  // exactly `bytes` bytes on the heap (malloc(0) may be null: never dereferenced then)
  unsigned char* buf = static_cast<unsigned char*>(std::malloc(bytes > 0 ? (size_t)bytes : 1));
  if (bytes > 0) std::memset(buf, 0x5a, (size_t)bytes);
  const long lines = ra_lines(bytes);
  CHECK(lines == (bytes >= 4 ? (bytes - 4) / 128 + 1 : 0), "bytes %ld", bytes);
  std::vector<unsigned char> hit((size_t)(bytes / 128 + 2), 0);
  unsigned long sum = 0;
  long touched = 0, max_line = -1;
  for (int wg = 0; wg < nwg; ++wg)
    for (int s = 0; s < slots; ++s) {
      const long first = ra_slot_first_line(nwg, wg, s);
      for (int lane = 0; lane < 64; ++lane) {
        const long off = ra_offset(bytes, nwg, slots, wg, s, lane);
        // the device half: the slot is skipped when its first line is past the range, a lane when its own line is
        const bool dev = first < lines && lane < lines - first;
        CHECK(dev == (off >= 0), "bytes %ld nwg %d slots %d wg %d slot %d lane %d", bytes, nwg, slots, wg, s, lane);
        if (off < 0) continue;
        CHECK(off == (first + lane) * 128, "decomposition: bytes %ld off %ld", bytes, off);
        CHECK(off % 128 == 0 && off + 4 <= bytes, "bytes %ld off %ld", bytes, off);
        if (off + 4 > bytes) continue;
        unsigned v;
        std::memcpy(&v, buf + off, 4);                      // the touch itself
        sum += v;
        const long line = off / 128;
        CHECK(!hit[(size_t)line], "bytes %ld line %ld touched twice", bytes, line);
        hit[(size_t)line] = 1;
        ++touched;
        if (line > max_line) max_line = line;
      }
    }
  const long cap = (long)slots * 64 * nwg;
  if (cap >= lines) CHECK(touched == lines, "coverage: bytes %ld nwg %d slots %d touched %ld of %ld", bytes, nwg, slots, touched, lines);
  else CHECK(touched == cap, "prefix: bytes %ld nwg %d slots %d touched %ld of capacity %ld", bytes, nwg, slots, touched, cap);
  CHECK(max_line == touched - 1, "not a prefix: bytes %ld nwg %d slots %d", bytes, nwg, slots);   // lines 0 .. touched-1, each once
  CHECK(ra_slots(bytes, nwg, slots) <= slots && (long)ra_slots(bytes, nwg, 1 << 20) * 64 * nwg >= lines, "ra_slots: bytes %ld nwg %d", bytes, nwg);
  // arguments outside the plan never yield an offset
  CHECK(ra_offset(bytes, nwg, slots, nwg, 0, 0) < 0 && ra_offset(bytes, nwg, slots, 0, slots, 0) < 0 && ra_offset(bytes, nwg, slots, 0, 0, 64) < 0 &&
        ra_offset(bytes, nwg, slots, -1, 0, 0) < 0 && ra_offset(bytes, 0, slots, 0, 0, 0) < 0, "out-of-plan arguments");
  std::free(buf);
  return sum;
}

int main() {
  const long sizes[] = {0, 4, 127, 128, 129, 8191, 8193, 2097152, 6291456};
  const int wgs[] = {1, 7, 256}, slots[] = {1, 4, 16};
  unsigned long sum = 0;
  int cases = 0;
  for (long b : sizes)
    for (int g : wgs)
      for (int s : slots) { sum += run_case(b, g, s); ++cases; }
  for (long b : {1L, 2L, 3L, -5L}) CHECK(ra_lines(b) == 0 && ra_offset(b, 1, 1, 0, 0, 0) < 0, "bytes %ld", b);

  // descriptor -> kernel argument: the chain's ranges (D = 1024: Wqkv 6 MiB, Wo 2 MiB) are covered by the device plan of 256 workgroups x kRaMaxSlots
  {
    const long bq = 3L * 1024 * 1024 * 2, bo = 1024L * 1024 * 2;
    char* wq = static_cast<char*>(std::malloc((size_t)bq));
    char* wo = static_cast<char*>(std::malloc((size_t)bo));
    RaRanges r = ra_make(wq, bq, wo, bo);
    CHECK(r.ptr[0] == wq && r.bytes[0] == bq && r.ptr[1] == wo && r.bytes[1] == bo, "ra_make");
    CHECK(ra_slots(bq, 256, kRaMaxSlots) == 3 && ra_slots(bo, 256, kRaMaxSlots) == 1, "slots %d %d", ra_slots(bq, 256, kRaMaxSlots), ra_slots(bo, 256, kRaMaxSlots));
    CHECK((long)kRaMaxSlots * 64 * 256 >= ra_lines(bq), "plan capacity");
    r = ra_make(nullptr, bq, wo, 0);
    CHECK(!r.ptr[0] && !r.bytes[0] && !r.ptr[1] && !r.bytes[1], "null / empty ranges are refused");
    r = ra_make(wq + 2, 64, wo, 3);
    CHECK(!r.ptr[0] && !r.bytes[0] && !r.ptr[1] && !r.bytes[1], "misaligned / sub-dword ranges are refused");
    std::free(wq); std::free(wo);
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("runahead plan OK: %d cases (checksum %lu)\n", cases, sum);
  return 0;
}
