// own_sim.cpp -- the owners of pybitmessage_amd/csrc/bmpow_own.h instantiated over a counting stand-in
// for the HIP runtime (no GPU, no HIP): every allocation is released exactly once and on the device it
// was made for, moves empty their source, grow() below the capacity allocates nothing, a failing grow()
// leaves the owner empty, retiring (a move into a vector) releases nothing until the vector is cleared,
// and with the exit flag set destructors release nothing.  The wiping owner (WipeBuf) on top: one zeroing
// of the whole capacity on the owner's device right before each release, and none where nothing is
// released.  Built with g++ under ASan + UBSan + LSan by
// tests/test_native.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../pybitmessage_amd/csrc/bmpow_own.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

// The stand-in: malloc / free, with a ledger of what is live (pointer -> device), counts, and a switch
// that makes the next allocation fail.
struct Fake {
  using err_t = int;
  static constexpr err_t ok = 0;
  static std::map<void*, int> live;
  static int allocs, frees, wrong_dev, unknown;
  static bool fail_next;
  // the wiping owner's ledger: every zeroing (pointer, device, bytes) and the pointers freed, in order
  struct Zero {
    void* p;
    int dev;
    size_t bytes;
  };
  static std::vector<Zero> zeros;
  static std::vector<void*> freed;
  static int zero_not_live;
  static void zero(int dev, void* p, size_t bytes) {
    if (!live.count(p)) ++zero_not_live;  // zeroing after the free, or of a pointer never allocated
    else std::memset(p, 0, bytes);        // the whole range is the allocation's (ASan)
    zeros.push_back({p, dev, bytes});
  }
  static err_t alloc(int dev, size_t bytes, unsigned, void** p, void** d) {
    if (fail_next) {
      fail_next = false;
      return 2;
    }
    *p = *d = std::malloc(bytes ? bytes : 1);
    live[*p] = dev;
    ++allocs;
    return ok;
  }
  static void free(int dev, void* p) {
    auto it = live.find(p);
    if (it == live.end()) {
      ++unknown;  // a double release, or a pointer never allocated
      return;
    }
    if (it->second != dev) ++wrong_dev;
    live.erase(it);
    std::free(p);
    freed.push_back(p);
    ++frees;
  }
  static void reset_counts() {
    allocs = frees = wrong_dev = unknown = zero_not_live = 0;
    zeros.clear();
    freed.clear();
  }
};
std::map<void*, int> Fake::live;
int Fake::allocs = 0, Fake::frees = 0, Fake::wrong_dev = 0, Fake::unknown = 0;
bool Fake::fail_next = false;
std::vector<Fake::Zero> Fake::zeros;
std::vector<void*> Fake::freed;
int Fake::zero_not_live = 0;

using Buf = bmown::Buf<long, Fake>;
using WBuf = bmown::WipeBuf<long, Fake>;

struct Retirable {  // as the engine's launch buffers: several owners retired together
  Buf a, b;
  size_t cap = 0;
};

void balanced() {
  CHECK(Fake::live.empty());
  CHECK(Fake::allocs == Fake::frees);
  CHECK(Fake::wrong_dev == 0);
  CHECK(Fake::unknown == 0);
}

void test_release_once_on_its_device() {
  Fake::reset_counts();
  {
    Buf x, y;
    CHECK(!x && x.cap() == 0 && x.get() == nullptr);
    CHECK(x.alloc(3, 100) == Fake::ok);
    CHECK(y.alloc(5, 7) == Fake::ok);
    CHECK(x && x.cap() == 100 && x.dev() == 3 && Fake::live[x.get()] == 3);
    CHECK(y.dev() == 5 && Fake::live[y.get()] == 5);
    x[99] = 42;  // the whole capacity is addressable (ASan)
    CHECK(x.dptr() == x.get());
    x.reset();
    CHECK(!x && x.cap() == 0 && x.dev() == -1 && Fake::frees == 1);
    x.reset();  // idempotent
    CHECK(Fake::frees == 1);
    CHECK(x.alloc(4, 10) == Fake::ok);  // reusable; and alloc over a held buffer releases it first
    CHECK(x.alloc(6, 20) == Fake::ok);
    CHECK(Fake::allocs == 4 && Fake::frees == 2 && x.dev() == 6);
  }
  CHECK(Fake::allocs == 4 && Fake::frees == 4);
  balanced();
}

void test_move() {
  Fake::reset_counts();
  {
    Buf x;
    CHECK(x.alloc(1, 8) == Fake::ok);
    long* p = x.get();
    Buf y(std::move(x));
    CHECK(!x && x.get() == nullptr && x.cap() == 0 && x.dev() == -1);
    CHECK(y.get() == p && y.cap() == 8 && y.dev() == 1);
    Buf z;
    CHECK(z.alloc(2, 4) == Fake::ok);
    z = std::move(y);  // releases z's own buffer (on device 2), takes y's
    CHECK(!y && z.get() == p && z.dev() == 1 && Fake::frees == 1);
    Buf& zr = z;
    z = std::move(zr);  // self-move keeps the buffer
    CHECK(z.get() == p && Fake::frees == 1);
  }
  CHECK(Fake::allocs == 2 && Fake::frees == 2);
  balanced();
}

void test_grow() {
  Fake::reset_counts();
  {
    Buf x;
    CHECK(x.grow(0, 16) == Fake::ok && x.cap() == 16 && Fake::allocs == 1);
    long* p = x.get();
    CHECK(x.grow(0, 16) == Fake::ok && x.grow(0, 3) == Fake::ok);  // below the capacity: nothing
    CHECK(x.get() == p && x.cap() == 16 && Fake::allocs == 1 && Fake::frees == 0);
    CHECK(x.grow(0, 17) == Fake::ok && x.cap() == 17);  // exactly what the caller's policy chose
    CHECK(Fake::allocs == 2 && Fake::frees == 1);
    Fake::fail_next = true;
    CHECK(x.grow(0, 64) != Fake::ok);  // the old buffer is released once, the owner is left empty
    CHECK(!x && x.cap() == 0 && x.get() == nullptr && x.dev() == -1);
    CHECK(Fake::allocs == 2 && Fake::frees == 2);
    CHECK(x.grow(0, 64) == Fake::ok && x.cap() == 64);  // and the next call starts over
  }
  CHECK(Fake::allocs == 3 && Fake::frees == 3);
  balanced();
}

void test_retire() {
  Fake::reset_counts();
  {
    std::vector<Retirable> retired;
    Retirable m;
    for (int round = 0; round < 5; ++round) {  // the vector reallocates on the way: still nothing released
      CHECK(m.a.alloc(round, 4) == Fake::ok && m.b.alloc(round, 4) == Fake::ok);
      m.cap = 4;
      retired.push_back(std::move(m));
      CHECK(!m.a && !m.b);
      CHECK(Fake::frees == 0);
    }
    CHECK(Fake::allocs == 10 && Fake::live.size() == 10);
    retired.clear();
    CHECK(Fake::frees == 10);
  }
  balanced();
}

void test_exit_flag() {
  Fake::reset_counts();
  std::vector<void*> leaked;
  {
    Buf x, y;
    CHECK(x.alloc(0, 4) == Fake::ok && y.alloc(1, 4) == Fake::ok);
    leaked = {x.get(), y.get()};
    bmown::g_exiting.store(true);
    y.reset();  // forgets, releases nothing
    CHECK(!y);
  }
  CHECK(Fake::frees == 0 && Fake::live.size() == 2);
  bmown::g_exiting.store(false);
  for (void* p : leaked) {  // the process would be gone by now; the test tidies up for LeakSanitizer
    Fake::live.erase(p);
    std::free(p);
  }
}

// release number k (counted from 0) was of pointer p, and was preceded by exactly one zeroing: of p, on
// device dev, of cap elements, while p was still live
void wiped_before_free(size_t k, void* p, int dev, size_t cap) {
  CHECK(Fake::freed.size() == k + 1 && Fake::zeros.size() == k + 1);
  if (Fake::freed.size() != k + 1 || Fake::zeros.size() != k + 1) return;
  CHECK(Fake::freed[k] == p);
  CHECK(Fake::zeros[k].p == p && Fake::zeros[k].dev == dev && Fake::zeros[k].bytes == cap * sizeof(long));
  CHECK(Fake::zero_not_live == 0);
}

void test_wipe_before_every_release() {
  Fake::reset_counts();
  {
    WBuf x;
    CHECK(x.alloc(3, 10) == Fake::ok);
    x[9] = 7;
    void* p = x.get();
    x.reset();  // reset
    wiped_before_free(0, p, 3, 10);
    CHECK(x.alloc(4, 20) == Fake::ok);
    p = x.get();
    CHECK(x.alloc(5, 30) == Fake::ok);  // a second alloc
    wiped_before_free(1, p, 4, 20);
    p = x.get();
    CHECK(x.grow(5, 31) == Fake::ok && x.cap() == 31);  // a grow that reallocates
    wiped_before_free(2, p, 5, 30);
    WBuf y;
    CHECK(y.alloc(6, 8) == Fake::ok);
    p = y.get();
    void* q = x.get();
    y = std::move(x);  // move-assignment over a live buffer: y's old one goes, x's is taken as it is
    wiped_before_free(3, p, 6, 8);
    CHECK(y.get() == q && y.cap() == 31 && y.dev() == 5 && !x);
    p = q;
    {
      WBuf z(std::move(y));  // destruction, of the owner the buffer moved into
      CHECK(Fake::zeros.size() == 4);
    }
    wiped_before_free(4, p, 5, 31);
  }
  CHECK(Fake::zeros.size() == 5 && Fake::frees == 5);  // the moved-from owners died without a zeroing
  balanced();
}

void test_no_wipe_without_a_release() {
  Fake::reset_counts();
  {
    WBuf empty;
    empty.reset();  // an empty owner
    WBuf x;
    CHECK(x.grow(0, 16) == Fake::ok);
    CHECK(x.grow(0, 16) == Fake::ok && x.grow(0, 3) == Fake::ok);  // a grow within the capacity
    CHECK(Fake::zeros.empty() && Fake::frees == 0);
    WBuf y(std::move(x));
    x.reset();  // a moved-from owner
    CHECK(Fake::zeros.empty() && Fake::frees == 0);
    Fake::fail_next = true;
    void* p = y.get();
    CHECK(y.grow(0, 64) != Fake::ok && !y);  // a failing grow still released the old buffer: wiped first
    wiped_before_free(0, p, 0, 16);
  }
  CHECK(Fake::zeros.size() == 1 && Fake::frees == 1);
  balanced();
  // after the exit flag: nothing is zeroed, nothing is freed
  Fake::reset_counts();
  void* leaked = nullptr;
  {
    WBuf x;
    CHECK(x.alloc(2, 4) == Fake::ok);
    leaked = x.get();
    bmown::g_exiting.store(true);
  }
  CHECK(Fake::zeros.empty() && Fake::frees == 0 && Fake::live.size() == 1);
  bmown::g_exiting.store(false);
  Fake::live.erase(leaked);
  std::free(leaked);
}

}  // namespace

int main() {
  test_release_once_on_its_device();
  test_move();
  test_grow();
  test_retire();
  test_exit_flag();
  test_wipe_before_every_release();
  test_no_wipe_without_a_release();
  if (g_failed) {
    std::fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  std::fprintf(stderr, "all owner checks passed\n");
  return 0;
}
