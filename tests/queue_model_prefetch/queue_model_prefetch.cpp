// CPU model of the queue launches' scheduling protocol WITH the early take (csrc/mre_kernels.hip: queue_take, QueueItem,
// step_body<QUEUE>) -- test infrastructure, not the product.  tests/queue_model/queue_model.cpp models the serial
// protocol; this one is the same lists, counters and order of atomic operations, and a wave that
//   * takes its NEXT item in the middle of the current one (one look, never a wait) and reads the env's rows into
//     "registers" right behind the acquire,
//   * looks once more at the top of its loop, after it has listed its own env, when the early take found nothing
//     (large waves of the waiting launch wait there, as they always did),
//   * keeps an item it took early when the current tick is abandoned (hand-over to the large shard).
// An env's "rows" are one word (ticks stepped so far) in plain memory, written before the release of the listing and
// read after the acquire of the take.  Checked: the rows an item was taken with are the rows of its tick (nothing stale,
// nothing taken before it was stored), a wave never takes the env it is holding, every (env, tick) is stepped exactly
// once and per env in order, an env that was handed over is only ever stepped by large threads afterwards, every thread
// terminates, and the count of finished envs ends at N.
//
//   queue_model_prefetch N T waves shards lw overflow_per_mille mode early seed
//     mode  0: the waiting large launch beside the compact threads; 1: alone BEFORE them (serialised dispatch)
//     early bit 0: compact threads take early; bit 1: large threads do (0: the serial take of the PGS kernels)
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

static int N, T, WAVES, S, SL, LW, OVF, EARLY;
static std::vector<std::atomic<int>> head, tail, buf;
static std::atomic<int> done{0}, started{0}, err{0};
static std::vector<int> rows;                  // plain memory: ticks stepped so far
static std::vector<uint8_t> moved;             // plain memory, travels with the rows
static std::vector<std::atomic<int>> stepped;  // [N * T]
static std::vector<uint8_t> large_flag;
static int cap, capl, stride;
static uint64_t seed;

static uint64_t mix(uint64_t x) { x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); }
static bool overflows(int env, int tick) { return (int)(mix(seed ^ ((uint64_t)env << 20) ^ (uint64_t)tick) % 1000) < OVF; }
static void work(int env, int tick, int part) { volatile unsigned x = 0; const unsigned n = 25 + (unsigned)(mix(seed + env * 131 + tick * 2 + part) % 200); for (unsigned i = 0; i < n; i++) x += i; }

static std::atomic<int>* bucket(int t, int sh) {
  return &buf[(size_t)t * stride + (sh < S ? (size_t)sh * cap : (size_t)S * cap + (size_t)(sh - S) * capl)];
}

// queue_pop_shard: 1 taken, 0 nothing ready, -1 error
static int pop_shard(int sh, int& env, int& tick) {
  const bool order0 = sh < S;
  const int n0 = (N - sh + S - 1) / S;
  for (;;) {
    int t = -1, ht = 0;
    for (int b = 0; b < T; b++) {
      const int h = head[sh * T + b].load(std::memory_order_relaxed);
      const int tl = (b == 0 && order0) ? n0 : tail[sh * T + b].load(std::memory_order_relaxed);
      if (h < tl) { t = b; ht = h; break; }
    }
    if (t < 0) return 0;
    int got = -1;
    if (t == 0 && order0) {
      const int i = head[sh * T].fetch_add(1, std::memory_order_relaxed);
      if (i < n0) got = sh + S * i;
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
  std::atomic_thread_fence(std::memory_order_release);   // (the device: write-through stores, every one waited for)
  const int i = tail[shard * T + tick].fetch_add(1, std::memory_order_relaxed);
  bucket(tick, shard)[i].store(env + 1, std::memory_order_relaxed);
}

struct Item { bool have = false; int env = 0, tick = 0, shard = 0, rows = 0; uint8_t moved = 0; };

// queue_take: queue_pop (`wait`: a large thread of the waiting launch, at the top of its loop), the acquire, the rows.
// False: a protocol error, the thread ends.
static bool take(int w, bool large, bool wait, Item& it) {
  it.have = false;
  if (large) {
    const int home = w % SL;
    for (unsigned idle = 0;; ++idle) {
      int r = 0;
      for (int k = 0; k < SL && r == 0; ++k) {
        const int sh = S + (home + k) % SL;
        r = pop_shard(sh, it.env, it.tick);
        if (r != 0) it.shard = sh;
      }
      if (r < 0) return false;
      if (r > 0) { it.have = true; break; }
      if (!wait || done.load(std::memory_order_relaxed) >= N) return true;
      if (idle > 2000u && started.load(std::memory_order_relaxed) == 0) return true;
      if (idle > (1u << 24)) return true;
      std::this_thread::yield();
    }
  } else {
    const int home = w % S;
    for (int k = 0; k < S && !it.have; ++k) {
      const int sh = (home + k) % S;
      const int r = pop_shard(sh, it.env, it.tick);
      if (r < 0) return false;
      if (r > 0) { it.have = true; it.shard = sh; }
    }
  }
  if (!it.have) return true;
  if (it.tick > 0 || large) std::atomic_thread_fence(std::memory_order_acquire);
  it.rows = rows[it.env]; it.moved = moved[it.env];   // the rows, into registers
  return true;
}

static void wave(int w, bool large, bool wait) {
  if (!large) started.fetch_add(1, std::memory_order_relaxed);
  const bool early = (EARLY & (large ? 2 : 1)) != 0;
  Item next;
  for (;;) {
    if (!next.have && !take(w, large, wait, next)) return;
    if (!next.have) return;
    const Item cur = next;
    next.have = false;
    const int env = cur.env, tick = cur.tick;
    if (!large && tick == 0 && large_flag[env]) continue;   // in the large shard's list
    // ---- one control tick, on the rows the item was taken with
    if (cur.rows != tick) { fprintf(stderr, "env %d taken for tick %d with rows at %d\n", env, tick, cur.rows); err = 2; return; }
    if (!large && cur.moved) { fprintf(stderr, "env %d stepped by a compact wave after its hand-over\n", env); err = 3; return; }
    work(env, tick, 0);
    if (early) {   // after the solver of the tick's last step: one look, no wait
      if (!take(w, large, false, next)) return;
      if (next.have && next.env == env) { fprintf(stderr, "env %d taken by the wave that holds it\n", env); err = 4; return; }
    }
    work(env, tick, 1);
    const bool hand_over = !large && overflows(env, tick);
    if (hand_over) {
      moved[env] = 1;
      push(env, tick, S + env % SL);   // the same tick again; an item taken early is kept and stepped next
      continue;
    }
    stepped[(size_t)env * T + tick].fetch_add(1, std::memory_order_relaxed);
    rows[env] = tick + 1;
    if (tick + 1 < T) push(env, tick + 1, cur.shard);
    else done.fetch_add(1, std::memory_order_relaxed);
  }
}

int main(int argc, char** argv) {
  if (argc < 10) { fprintf(stderr, "usage: queue_model_prefetch N T waves shards lw overflow_per_mille mode early seed\n"); return 2; }
  N = atoi(argv[1]); T = atoi(argv[2]); WAVES = atoi(argv[3]); S = atoi(argv[4]); LW = atoi(argv[5]); OVF = atoi(argv[6]);
  const int mode = atoi(argv[7]); EARLY = atoi(argv[8]); seed = strtoull(argv[9], nullptr, 10);
  SL = S > 1 ? (S + 1) / 2 : 1;
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
  for (int e = 0; e < N; e++) if (mix(seed * 7 + e) % 23 == 0) { large_flag[e] = 1; bucket(0, S + e % SL)[cnt[e % SL]++].store(e + 1); nl++; }
  for (int j = 0; j < SL; j++) tail[(S + j) * T].store(cnt[j]);
  std::vector<std::thread> th;
  for (int w = 0; w < LW; w++) th.emplace_back(wave, w, true, true);
  if (mode == 1) {   // the waiting large launch runs alone first and leaves (no compact wave shows up)
    for (auto& t : th) t.join();
    th.clear();
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
