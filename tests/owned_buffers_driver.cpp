// Driver of tests/test_owned_buffers.py: runs the owners of diaglib_amd/csrc/hip_owned.h against a counting fake runtime that
// can be told to fail its n-th allocation, and prints what it observed as "scenario.key=value" lines.  The assertions are in
// the Python file.  No ROCm header is involved: the fake below is the only `Api`.
#include <cstdio>
#include <cstdlib>
#include <set>
#include "../diaglib_amd/csrc/hip_owned.h"

struct FakeApi {
  using error_t = int;
  using event_t = void*;
  static constexpr int ok = 0;
  static inline long allocs = 0, frees = 0, host_allocs = 0, host_frees = 0, aliases = 0, ev_creates = 0, ev_destroys = 0;
  static inline long bad_release = 0;      // released something that was not live (double release, wild pointer)
  static inline long fail_alloc_at = 0;    // fail the n-th allocation request from now on (device and pinned count together)
  static inline bool fail_alias = false;
  static inline std::set<void*> live;
  static constexpr long ALIAS_OFFSET = 0x1000;

  static long calls() { return allocs + frees + host_allocs + host_frees + aliases + ev_creates + ev_destroys; }
  static int take(void** p, size_t bytes)
  {
    if (fail_alloc_at > 0 && --fail_alloc_at == 0) { *p = (void*)0xdead; return 2; }   // (garbage on failure: the owner must not keep it)
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    return 0;
  }
  static int give(void* p)
  {
    if (!live.erase(p)) { ++bad_release; return 1; }
    std::free(p);
    return 0;
  }
  static int alloc(void** p, size_t bytes, unsigned) { ++allocs; return take(p, bytes); }
  static int free(void* p) { ++frees; return give(p); }
  static int host_alloc(void** p, size_t bytes, bool) { ++host_allocs; return take(p, bytes); }
  static int host_free(void* p) { ++host_frees; return give(p); }
  static int host_alias(void** d, void* h)
  {
    ++aliases;
    if (fail_alias) { *d = (void*)0xdead; return 3; }
    *d = (char*)h + ALIAS_OFFSET;
    return 0;
  }
  static int event_create(void** e, unsigned) { ++ev_creates; return take(e, 1); }
  static int event_destroy(void* e) { ++ev_destroys; return give(e); }
  static void reset()
  {
    allocs = frees = host_allocs = host_frees = aliases = ev_creates = ev_destroys = bad_release = fail_alloc_at = 0;
    fail_alias = false;
  }
};

static const char* scenario = "";
static void say(const char* key, long v) { std::printf("%s.%s=%ld\n", scenario, key, v); }
static void begin(const char* name) { scenario = name; FakeApi::reset(); }
// allocations and releases of a finished scenario must balance, whatever happened in it
static void end() { say("live_at_exit", (long)FakeApi::live.size()); say("bad_release", FakeApi::bad_release); }

using Dev = DeviceBuffer<double, FakeApi>;
using Map = MappedHostBuffer<double, FakeApi>;
using Ev = BasicEvent<FakeApi>;

template <class B> static long releases();
template <> long releases<Dev>() { return FakeApi::frees; }
template <> long releases<Map>() { return FakeApi::host_frees; }
static bool aliased(const Dev&) { return true; }
static bool aliased(const Map& b) { return b.dev() == ((double*)b ? (double*)((char*)(double*)b + FakeApi::ALIAS_OFFSET) : nullptr); }

template <class B> static void buffer_scenarios(const char* grow, const char* noop, const char* move)
{
  begin(grow);
  {
    B b;
    say("first_ok", b.reserve(10) == 0 && (bool)b && b.capacity() == 10 && aliased(b));
    double* const old = b;
    FakeApi::fail_alloc_at = 1;
    say("regrow_failed", b.reserve(20) != 0);
    say("empty_after_failure", !b && (double*)b == nullptr && b.capacity() == 0 && aliased(b));
    say("old_released", releases<B>());
    say("old_still_live", (long)FakeApi::live.count(old));
    say("retry_ok", b.reserve(20) == 0 && (bool)b && b.capacity() == 20 && aliased(b));
    b[19] = 1.0;                           // (the sanitizer build checks that the block really has 20 elements)
    say("releases_before_exit", releases<B>());
  }
  say("releases_after_exit", releases<B>());
  end();

  begin(noop);
  {
    B b;
    (void)b.reserve(10);
    double* const p = b;
    const long c0 = FakeApi::calls();
    say("ok", b.reserve(10) == 0 && b.reserve(5) == 0 && b.reserve(0) == 0);
    say("runtime_calls", FakeApi::calls() - c0);
    say("unchanged", (double*)b == p && b.capacity() == 10);
  }
  end();

  begin(move);
  {
    B a, c;
    (void)a.reserve(10);
    (void)c.reserve(3);
    double* const p = a;
    B b(std::move(a));
    say("constructed", (double*)b == p && b.capacity() == 10 && !a && a.capacity() == 0 && aliased(b) && aliased(a));
    c = std::move(b);                      // releases c's own block, takes b's
    say("assigned", (double*)c == p && c.capacity() == 10 && !b && b.capacity() == 0 && aliased(c));
    say("releases_after_assignment", releases<B>());
    say("moved_from_regrows", a.reserve(4) == 0 && a.capacity() == 4);
  }
  say("releases_after_exit", releases<B>());   // c's first block, the moved block once, a's new block
  end();
}

int main()
{
  buffer_scenarios<Dev>("dev_grow", "dev_noop", "dev_move");
  buffer_scenarios<Map>("map_grow", "map_noop", "map_move");

  begin("map_alias");
  {
    Map b;
    (void)b.reserve(4);
    say("first", aliased(b) && b.dev() != nullptr);
    (void)b.reserve(4000);
    say("regrown", (double*)b != nullptr && aliased(b));
    say("alias_calls", FakeApi::aliases);
    FakeApi::fail_alias = true;
    say("alias_failed", b.reserve(8000) != 0);
    say("empty_after_failure", !b && (double*)b == nullptr && b.dev() == nullptr && b.capacity() == 0);
    FakeApi::fail_alias = false;
    say("retry_ok", b.reserve(8000) == 0 && aliased(b) && b.capacity() == 8000);
    Map u;                                 // not mapped: no alias is asked for
    const long a0 = FakeApi::aliases;
    say("unmapped", u.reserve(4, false) == 0 && (double*)u != nullptr && u.dev() == nullptr && FakeApi::aliases == a0);
  }
  end();

  begin("event");
  {
    Ev e;
    say("starts_empty", !e);
    FakeApi::fail_alloc_at = 1;
    say("create_failed", e.ensure(0) != 0 && !e);
    say("ensure_twice", e.ensure(0) == 0 && e.ensure(0) == 0 && (bool)e);
    say("creates", FakeApi::ev_creates);   // the failed one and one more
    say("destroys_before_exit", FakeApi::ev_destroys);
  }
  say("destroys_after_exit", FakeApi::ev_destroys);
  end();
  return 0;
}
