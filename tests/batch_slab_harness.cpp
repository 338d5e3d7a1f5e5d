// The host layer of the batched calls (dm-vio_amd/csrc/batch_slab.hpp: cursor, fixed-slab sizing, head check, repeat test, work counter) compiled by a plain host
// compiler with no HIP in sight.  Run as its own executable by tests/test_batch_slab_cpu.py; prints one line per failed check and "ok <n checks>" at the end.
#include <chrono>
#include <cstdio>
#include <string>

static std::string g_err;
static int failmsg(const std::string& m) { g_err = m; return -2; }
#include "batch_slab.hpp"

static int n_checks = 0, n_bad = 0;
#define CHECK(x) do { n_checks++; if (!(x)) { n_bad++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); } } while (0)

struct Odd { char c[37]; };   // a record of odd size

template <class T>
static void cursorCase() {
  const size_t counts[] = {0, 1, 63, 64, 65};
  for (size_t first : counts)
    for (size_t second : counts) {
      DmvCursor c;
      const size_t a = c.take<T>(first);
      const size_t mid = c.bytes();
      const size_t b = c.take<T>(second);
      CHECK(a == 0);
      CHECK(b == mid);                                   // a part starts where the one before ended ...
      CHECK(mid % 256 == 0 && c.bytes() % 256 == 0);     // ... on a 256-byte boundary
      CHECK(mid >= sizeof(T) * first && mid < sizeof(T) * first + 256);   // holds the part, wastes less than one granule
      CHECK(c.bytes() - b >= sizeof(T) * second && c.bytes() - b < sizeof(T) * second + 256);
      CHECK((first == 0) == (mid == 0));                 // nothing taken, nothing used
    }
}

// what a call packs, written out with the cursor as the calls do, against what creation reserves.  The kernel headers do not compile here, so the record sizes are made up
// and both sides go through the dmv* functions: this holds those functions to each other, and holds a call only as far as it packs with nothing else (the selector batch
// places window k's table at dmvSelLuts() + 1024 k by hand, inside the part that function took).
static void fixedSlabs() {
  const size_t trace_rec = 233, sel_rec = 389, ref_rec = 171, ba_rec = 77;   // odd record sizes: the sizing must not lean on a record being a multiple of anything
  const int max_hosts = 64;
  for (int max_windows : {1, 7, 65535}) {
    for (int W : {1, max_windows}) {
      {
        DmvCursor c;
        dmvRecords(c, trace_rec, W);
        for (int k = 0; k < W; k++) { const size_t at = dmvTraceTable(c, max_hosts); CHECK(at % 256 == 0); }
        CHECK(c.bytes() <= dmvTraceSlabBytes(trace_rec, max_windows, max_hosts));
        if (W == max_windows) CHECK(c.bytes() == dmvTraceSlabBytes(trace_rec, max_windows, max_hosts));
      }
      {
        DmvCursor c;
        dmvRecords(c, sel_rec, W);
        const size_t luts = dmvSelLuts(c, W);
        CHECK(luts >= sel_rec * W && c.bytes() >= luts + 1024 * (size_t)W);
        CHECK(c.bytes() <= dmvSelSlabBytes(sel_rec, max_windows));
      }
      for (int max_points : {1, 2000}) {
        const size_t total = (size_t)W * max_points;   // every window at max_points_per_window
        DmvCursor c;
        dmvRecords(c, ref_rec, W);
        const size_t pts = dmvRefPoints(c, total), ranks = dmvRefRanks(c, total);
        CHECK(pts % sizeof(float) == 0 && ranks >= pts + 16 * total && c.bytes() >= ranks + total);
        CHECK(c.bytes() <= dmvRefSlabBytes(ref_rec, ba_rec, max_windows, max_points));
        DmvCursor d;   // the from-BA form of the same slab
        dmvRecords(d, ref_rec, W);
        dmvRecords(d, ba_rec, W);
        CHECK(d.bytes() <= dmvRefSlabBytes(ref_rec, ba_rec, max_windows, max_points));
      }
    }
  }
}

static int repeated(std::initializer_list<int> ids) {
  static char pool[64];
  std::vector<const void*> p;
  for (int i : ids) p.push_back(pool + i);
  return dmvFirstRepeated(p.data(), (int)p.size());
}
struct Win { int pad; const char* handle; };

static void repeats() {
  CHECK(repeated({}) == -1);
  CHECK(repeated({5}) == -1);
  CHECK(repeated({5, 6}) == -1);
  CHECK(repeated({5, 5}) == 1);
  CHECK(repeated({9, 9, 1, 2, 3}) == 1);         // at the front
  CHECK(repeated({1, 9, 2, 9, 3}) == 3);         // in the middle
  CHECK(repeated({1, 2, 3, 9, 9}) == 4);         // at the end
  CHECK(repeated({3, 2, 1, 0, 3}) == 4);         // whatever the address order
  CHECK(repeated({7, 7, 7}) == 1);               // named three times: its second appearance
  CHECK(repeated({8, 2, 2, 8}) == 2);            // two repeats: the earlier by window index wins, not the lower address ...
  CHECK(repeated({2, 8, 8, 2}) == 2);
  CHECK(repeated({2, 8, 2, 8}) == 2);            // ... and not the handle that appeared first
  static char pool[8];
  const Win w[4] = {{0, pool + 1}, {0, pool + 2}, {0, pool + 1}, {0, nullptr}};
  CHECK(dmvFirstRepeated(w, 4, &Win::handle) == 2);
  CHECK(dmvFirstRepeated(w, 2, &Win::handle) == -1);
  // the largest batch a create function accepts plus one repeat: n log n, not the 2e9 comparisons of a double loop
  const int N = 65535;
  static char big[N];
  std::vector<const void*> p;
  for (int i = 0; i < N; i++) p.push_back(big + (size_t)((i * 7919ull) % N));   // distinct (7919 is prime and no factor of 65535), in scrambled address order
  CHECK(dmvFirstRepeated(p.data(), N) == -1);
  p.push_back(p[12345]);
  const auto t0 = std::chrono::steady_clock::now();
  CHECK(dmvFirstRepeated(p.data(), N + 1) == N);
  p[N] = p[N - 1]; p[N - 1] = p[100];
  CHECK(dmvFirstRepeated(p.data(), N + 1) == N - 1);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("dmvFirstRepeated: two passes over %d handles in %.1f ms\n", N + 1, ms);
}

static void heads() {
  int handle = 0, arr = 0;
  g_err.clear();
  CHECK(dmvBatchHead(&handle, 0, 4, nullptr, "call") == 0 && g_err.empty());   // W = 0 needs no array
  CHECK(dmvBatchHead(&handle, 4, 4, &arr, "call") == 0 && g_err.empty());
  CHECK(dmvBatchHead(nullptr, 1, 4, &arr, "call") != 0 && g_err == "call: null batch handle");
  CHECK(dmvBatchHead(&handle, -1, 4, &arr, "call") != 0 && g_err == "call: W is negative or larger than the batch's max_windows");
  CHECK(dmvBatchHead(&handle, 5, 4, &arr, "call") != 0 && g_err == "call: W is negative or larger than the batch's max_windows");
  CHECK(dmvBatchHead(&handle, 1, 4, nullptr, "call") != 0 && g_err == "call: the window array is NULL");
  CHECK(dmvBatchHead(nullptr, -1, 4, nullptr, "call") != 0 && g_err == "call: null batch handle");   // the order of the refusals: handle, W, array
  CHECK(dmvBatchHead(&handle, 9, 4, nullptr, "call") != 0 && g_err == "call: W is negative or larger than the batch's max_windows");
  const char* const own[3] = {" a", " b", " c"};   // a caller's own wording
  CHECK(dmvBatchHead(&handle, 1, 4, nullptr, "call", own) != 0 && g_err == "call c");
  CHECK(dmvBatchHead(&handle, 0, 4, nullptr, "call", own) == 0);
}

static void work() {
  DmvWork w;
  w.launches = 2; w.uploads = 1; w.downloads = 3; w.waits = 4;
  int l = -1, u = -1, d = -1, q = -1;
  w.report(&l, nullptr, &d, nullptr);
  CHECK(l == 2 && u == -1 && d == 3 && q == -1);
  w.report(nullptr, &u, nullptr, &q);
  CHECK(u == 1 && q == 4);
  w.clear();
  w.report(&l, &u, &d, &q);
  CHECK(l == 0 && u == 0 && d == 0 && q == 0);
}

int main() {
  cursorCase<char>(); cursorCase<float>(); cursorCase<double>(); cursorCase<Odd>();
  { DmvCursor c; CHECK(c.bytes() == 0); CHECK(c.takeBytes(257) == 0 && c.bytes() == 512); CHECK(dmvPad(0) == 0 && dmvPad(1) == 256 && dmvPad(256) == 256); }
  fixedSlabs();
  repeats();
  heads();
  work();
  if (n_bad) { printf("%d of %d checks failed\n", n_bad, n_checks); return 1; }
  printf("ok %d checks\n", n_checks);
  return 0;
}
