// CPU model of the queue launches' scheduling protocol (csrc/mre_kernels.hip: queue_pop_shard / queue_pop / queue_push,
// step_body<QUEUE>; csrc/mre_sched.cpp: launch_group_enqueue) -- test infrastructure, not the product.
//
// Threads stand for waves: `waves` compact ones in `shards` shards, `lw` large ones that wait (the launch enqueued first),
// and after all compact threads have left, `lw` large ones that do not wait (the launch behind the compact kernel).  The
// lists, counters and the order of the atomic operations are those of the device code; an env's "rows" are one word (the
// number of ticks it has been stepped) written with a plain store before the release and read with a plain load after the
// acquire.  A tick "overflows the compact capacities" where hash(env, tick) says so: the compact thread abandons it and
// lists the env in the large shard for the same tick.  Checked: every env is stepped through ticks 0 .. T-1 exactly once
// each and in order (a stale or torn hand-off shows as a wrong row), an env that was handed over is only ever stepped by
// large threads afterwards, every thread terminates, and the count of finished envs ends at N.
//
//   queue_model N T waves shards lw overflow_per_mille mode seed      mode 0: side by side; 1: the waiting large launch
//   alone BEFORE the compact threads start (serialised dispatch: it leaves after its bounded wait)
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

static int N, T, WAVES, S, SL, LW, OVF;
static std::vector<std::atomic<int>> head, tail, buf;   // [(S + 1) * T], [(S + 1) * T], [T * stride]
static std::atomic<int> done{0}, started{0}, err{0};
static std::vector<int> rows;                  // the env's "state rows": ticks stepped so far (plain memory)
static std::vector<uint8_t> moved;             // env was handed over (plain memory, travels with the rows)
static std::vector<std::atomic<int>> stepped;  // [N * T] how often (env, tick) was stepped
static std::vector<uint8_t> large_flag;        // host's flags at launch start
static int cap, capl, stride;
static uint64_t seed;

static uint64_t mix(uint64_t x) { x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); }
static bool overflows(int env, int tick) { return (int)(mix(seed ^ ((uint64_t)env << 20) ^ (uint64_t)tick) % 1000) < OVF; }
static void work(int env, int tick) { volatile unsigned x = 0; const unsigned n = 50 + (unsigned)(mix(seed + env * 131 + tick) % 400); for (unsigned i = 0; i < n; i++) x += i; }

static std::atomic<int>* bucket(int t, int sh) {
  return &buf[(size_t)t * stride + (sh < S ? (size_t)sh * cap : (size_t)S * cap + (size_t)(sh - S) * capl)];
}

// queue_pop_shard: 1 taken, 0 nothing ready, -1 error
static int pop_shard(int sh, int& env, int& tick) {
  const bool order0 = sh < S;
  const int n0 = (N - sh + S - 1) / S;
  for (;;) {
    int t = -1, ht = 0;
    for (int b = 0; b < T; b++) {   // (one lane per bucket on the device: the lowest ready bucket)
      const int h = head[sh * T + b].load(std::memory_order_relaxed);
      const int tl = (b == 0 && order0) ? n0 : tail[sh * T + b].load(std::memory_order_relaxed);
      if (h < tl) { t = b; ht = h; break; }
    }
    if (t < 0) return 0;
    int got = -1;
    if (t == 0 && order0) {
      const int i = head[sh * T].fetch_add(1, std::memory_order_relaxed);
      if (i < n0) got = sh + S * i;   // (identity dispatch order)
    } else {
      int expect = ht;
      if (head[sh * T + t].compare_exchange_strong(expect, ht + 1, std::memory_order_relaxed)) {
        int v = bucket(t, sh)[ht].load(std::memory_order_relaxed);
        for (unsigned spin = 0; v == 0; ++spin) {
          if (spin > (1u << 26)) { err = 1; return -1; }
          std::this_thread::yield();
          v = bucket(t, sh)[ht].load(std::memory_order_relaxed);
        }
        got = v - 1;
      }
    }
    if (got < 0) continue;
    env = got; tick = t;
    return 1;
  }
}
static void push(int env, int tick, int shard) {
  std::atomic_thread_fence(std::memory_order_release);
  const int i = tail[shard * T + tick].fetch_add(1, std::memory_order_relaxed);
  bucket(tick, shard)[i].store(env + 1, std::memory_order_relaxed);
}

static void wave(int w, bool large, bool wait) {
  if (!large) started.fetch_add(1, std::memory_order_relaxed);
  for (;;) {
    int env = 0, tick = 0, shard = S;
    bool have = false;
    if (large) {
      const int home = w % SL;
      for (unsigned idle = 0;; ++idle) {
        int r = 0;
        for (int k = 0; k < SL && r == 0; ++k) {
          const int sh = S + (home + k) % SL;
          r = pop_shard(sh, env, tick);
          if (r != 0) shard = sh;
        }
        if (r < 0) return;
        if (r > 0) { have = true; break; }
        if (!wait || done.load(std::memory_order_relaxed) >= N) return;
        if (idle > 2000u && started.load(std::memory_order_relaxed) == 0) return;   // no compact wave in sight: leave
        if (idle > (1u << 24)) return;
        std::this_thread::yield();
      }
    } else {
      const int home = w % S;
      for (int k = 0; k < S && !have; ++k) {
        const int sh = (home + k) % S;
        const int r = pop_shard(sh, env, tick);
        if (r < 0) return;
        if (r > 0) { have = true; shard = sh; }
      }
    }
    if (!have) return;
    if (tick > 0 || large) std::atomic_thread_fence(std::memory_order_acquire);
    if (!large && tick == 0 && large_flag[env]) continue;   // in the large shard's list
    // ---- one control tick
    if (rows[env] != tick) { fprintf(stderr, "env %d taken for tick %d with rows at %d\n", env, tick, rows[env]); err = 2; return; }
    if (!large && moved[env]) { fprintf(stderr, "env %d stepped by a compact wave after its hand-over\n", env); err = 3; return; }
    work(env, tick);
    const bool hand_over = !large && overflows(env, tick);
    if (hand_over) {
      moved[env] = 1;                 // (q_acc: travels with the env)
      push(env, tick, S + env % SL);  // the same tick again, with the large capacities
      continue;
    }
    stepped[(size_t)env * T + tick].fetch_add(1, std::memory_order_relaxed);
    rows[env] = tick + 1;             // store the rows
    if (tick + 1 < T) push(env, tick + 1, shard);
    else done.fetch_add(1, std::memory_order_relaxed);
  }
}

int main(int argc, char** argv) {
  if (argc < 9) { fprintf(stderr, "usage: queue_model N T waves shards lw overflow_per_mille mode seed\n"); return 2; }
  N = atoi(argv[1]); T = atoi(argv[2]); WAVES = atoi(argv[3]); S = atoi(argv[4]); LW = atoi(argv[5]); OVF = atoi(argv[6]);
  const int mode = atoi(argv[7]); seed = strtoull(argv[8], nullptr, 10);
  SL = S > 1 ? (S + 1) / 2 : 1;   // (the library: 16 compact shards, 8 large ones)
  cap = (N + S - 1) / S; capl = (N + SL - 1) / SL; stride = S * cap + SL * capl;
  head = std::vector<std::atomic<int>>((S + SL) * T); tail = std::vector<std::atomic<int>>((S + SL) * T);
  buf = std::vector<std::atomic<int>>((size_t)T * stride);
  for (auto& x : head) x = 0;
  for (auto& x : tail) x = 0;
  for (auto& x : buf) x = 0;
  rows.assign(N, 0); moved.assign(N, 0); large_flag.assign(N, 0);
  stepped = std::vector<std::atomic<int>>((size_t)N * T);
  for (auto& x : stepped) x = 0;
  int nl = 0;
  std::vector<int> cnt(SL, 0);
  for (int e = 0; e < N; e++) if (mix(seed * 7 + e) % 23 == 0) { large_flag[e] = 1; bucket(0, S + e % SL)[cnt[e % SL]++].store(e + 1); nl++; }   // the host's lists
  for (int j = 0; j < SL; j++) tail[(S + j) * T].store(cnt[j]);
  std::vector<std::thread> th;
  if (mode == 1) {   // the waiting large launch runs alone first and leaves (no compact wave shows up)
    for (int w = 0; w < LW; w++) th.emplace_back(wave, w, true, true);
    for (auto& t : th) t.join();
    th.clear();
  } else {
    for (int w = 0; w < LW; w++) th.emplace_back(wave, w, true, true);
  }
  std::vector<std::thread> comp;
  for (int w = 0; w < WAVES; w++) comp.emplace_back(wave, w, false, false);
  for (auto& t : comp) t.join();
  std::vector<std::thread> sweep;   // behind the compact kernel: the large kernel once more, not waiting
  for (int w = 0; w < (LW > 0 ? LW : 1); w++) sweep.emplace_back(wave, w, true, false);
  for (auto& t : sweep) t.join();
  for (auto& t : th) t.join();
  if (err) { printf("FAIL protocol error %d\n", err.load()); return 1; }
  long bad = 0, handed = 0;
  for (int e = 0; e < N; e++) {
    handed += moved[e];
    if (rows[e] != T) bad++;
    for (int t = 0; t < T; t++) if (stepped[(size_t)e * T + t] != 1) bad++;
  }
  if (bad || done != N) { printf("FAIL %ld wrong entries, done %d of %d\n", bad, done.load(), N); return 1; }
  printf("OK %d envs x %d ticks, %d flagged large, %ld handed over\n", N, T, nl, handed);
  return 0;
}
