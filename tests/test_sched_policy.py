"""The launch scheduler's rules (csrc/mre_policy.h) on the CPU: tests/sched_policy/sched_policy.cpp reads cases on stdin,
applies the rule and prints what it decided.  Every expected value below is worked out from the rule's text (DESIGN.md,
the comments of mre_policy.h), never taken from the program."""
import itertools
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# compact capacities (csrc/mre_dev.h): contacts, constraint rows, robot rows (PGS / Newton), cube-cube contacts
NCON, NEFC, NRROW, NPP = 32, 112, {False: 62, True: 69}, 8
RING, NSTAGE = 4, 5


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sched_policy") / "sched_policy")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(HERE, "sched_policy", "sched_policy.cpp"), "-o", exe])

    def run(mode, text):
        out = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (mode, out.stdout[-200:], out.stderr[-500:])
        return out.stdout.split("\n")[:-1]
    return run


def record(li0, ncon=0, nefc=0, nrrow=0, npp=0, duration=0):
    """StepArgs::launch_info: {overflow word, max ncon | duration << 16, max nefc, max robot rows | max cube-cube << 16}"""
    return [li0, ncon | (duration << 16), nefc, nrrow | (npp << 16)]


def caps(newton):
    return {"ncon": NCON, "nefc": NEFC, "nrrow": NRROW[newton], "npp": NPP}


def rule(li0, marks, flag, newton, compact_only, large_only):
    """DESIGN.md, capacity fallback: (action, flag afterwards) for one env."""
    c = caps(newton)
    if li0 < 0:                                    # not part of the launch (-1) or waiting for its re-run (-2)
        return "none", flag
    if li0 & 4 and not flag:                       # a queue launch moved it to the large kernel itself
        return "handed_over", 1
    if li0 == 1:                                   # overflowed the compact kernel
        return "rerun", 1
    if not flag:                                   # within 1/8 of a compact capacity: promote (unless compact only)
        near = any(8 * marks[k] > 7 * c[k] for k in c)
        return ("promote", 1) if near and not compact_only else ("none", 0)
    below = all(8 * marks[k] <= 5 * c[k] for k in c)   # a large env that did not overflow and is at 5/8 or below: demote
    return ("demote", 0) if li0 == 0 and below and not large_only else ("none", 1)


def old_synchronous_rule(li0, marks, flag, newton, compact_only, large_only):
    """What the synchronous path carried before it shared the rule above: no `moved` bit, any overflow of an unflagged env
    is a re-run, a flagged env is only ever demoted."""
    c = caps(newton)
    if li0 < 0:
        return "none", flag
    if not flag:
        if li0 > 0:
            return "rerun", 1
        near = any(8 * marks[k] > 7 * c[k] for k in c)
        return ("promote", 1) if near and not compact_only else ("none", 0)
    below = all(8 * marks[k] <= 5 * c[k] for k in c)
    return ("demote", 0) if li0 == 0 and below and not large_only else ("none", 1)


def mark_settings(newton):
    """each high-water mark one below, at and one above its 7/8 and its 5/8 threshold, the other three at zero"""
    out = [dict(ncon=0, nefc=0, nrrow=0, npp=0)]
    for k, cap in caps(newton).items():
        for num in (7, 5):
            at = num * cap // 8
            for v in (at - 1, at, at + 1):
                out.append({**out[0], k: v})
    return out


def test_decision_table(policy):
    rows = []
    for newton in (False, True):
        for li0, flag, co, lo, marks in itertools.product((-2, -1, 0, 1, 2, 4, 6), (0, 1), (0, 1), (0, 1), mark_settings(newton)):
            rows.append((li0, marks, flag, newton, co, lo))
    assert len(rows) == 2 * 7 * 2 * 2 * 2 * 25
    text = "".join("%d %d %d %d %d %d %d %d\n" % (*record(li0, **m), flag, newton, co, lo) for li0, m, flag, newton, co, lo in rows)
    got = policy("decide", text)
    assert len(got) == len(rows)
    differ = set()
    for r, g in zip(rows, got):
        action, after = rule(*r)
        assert g == "%s %d" % (action, after), (r, g)
        # a synchronous launch runs an env on the kernel its HOST flag names: an unflagged env reports -1, 0 or 1, a flagged
        # one -1, 0 or 2, and no bit 2 -- on those records the shared rule is the one the synchronous path used to carry
        li0, flag = r[0], r[2]
        if li0 in ((-2, -1, 0, 2) if flag else (-2, -1, 0, 1)):
            assert old_synchronous_rule(*r) == (action, after), r
        elif old_synchronous_rule(*r) != (action, after):
            differ.add((li0, flag))
    # ... and these are the records it could never see, on which the two would have parted
    assert differ == {(2, 0), (4, 0), (6, 0), (1, 1)}


# the thresholds as numbers: (mark, solver, value) -> what an unflagged env with li0 = 0 / a flagged one with li0 = 0 does
@pytest.mark.parametrize("mark, newton, value, unflagged, flagged", [
    ("ncon", 0, 28, "none 0", "none 1"), ("ncon", 0, 29, "promote 1", "none 1"),       # 8 * 29 = 232 > 224
    ("nefc", 0, 98, "none 0", "none 1"), ("nefc", 0, 99, "promote 1", "none 1"),       # 8 * 99 = 792 > 784
    ("nrrow", 0, 54, "none 0", "none 1"), ("nrrow", 0, 55, "promote 1", "none 1"),     # PGS: 62 rows, 440 > 434
    ("nrrow", 1, 55, "none 0", "none 1"), ("nrrow", 1, 60, "none 0", "none 1"),        # Newton: 69 rows, 480 <= 483
    ("nrrow", 1, 61, "promote 1", "none 1"),                                           # 488 > 483
    ("npp", 0, 7, "none 0", "none 1"), ("npp", 0, 8, "promote 1", "none 1"),           # 8 * 7 = 56 is not > 56
    ("ncon", 0, 20, "none 0", "demote 0"), ("ncon", 0, 21, "none 0", "none 1"),        # 160 <= 160
    ("nefc", 0, 70, "none 0", "demote 0"), ("nefc", 0, 71, "none 0", "none 1"),        # 560 <= 560
    ("nrrow", 0, 38, "none 0", "demote 0"), ("nrrow", 0, 39, "none 0", "none 1"),      # PGS: 304 <= 310 < 312
    ("nrrow", 1, 43, "none 0", "demote 0"), ("nrrow", 1, 44, "none 0", "none 1"),      # Newton: 344 <= 345 < 352
    ("npp", 0, 5, "none 0", "demote 0"), ("npp", 0, 6, "none 0", "none 1"),            # 40 <= 40
])
def test_decision_thresholds_as_numbers(policy, mark, newton, value, unflagged, flagged):
    rec = record(0, **{mark: value}, duration=123)
    got = policy("decide", "".join("%d %d %d %d %d %d 0 0\n" % (*rec, flag, newton) for flag in (0, 1)))
    assert got == [unflagged, flagged]


def sort_input(total, lo, n, records, order):
    return "%d %d %d\n%s\n%s\n" % (total, lo, n, " ".join(str(w) for r in records for w in r), " ".join(map(str, order)))


def test_sort_longest_first_is_stable_and_stays_inside_its_range(policy):
    # 24 envs, the range is [4, 20); the longest duration is 255, so an env's bucket is its duration
    absent, waiting = [-1, -1, -1, -1], [-2, -1, -1, -1]
    durations = {4: 5, 5: 255, 6: 5, 7: absent, 8: 100, 9: 100, 10: 7, 11: 255, 12: 0, 13: 3, 14: 100, 15: 5, 16: waiting,
                 17: 200, 18: 1, 19: 7}
    records = [record(0, ncon=9, duration=30000)] * 4                      # outside the range: must not count for kmax
    records += [d if isinstance(d, list) else record(0, ncon=31, duration=d) for d in (durations[i] for i in range(4, 20))]
    records += [record(1, duration=20000)] * 4
    order = [100 + i for i in range(24)]
    got = policy("sort", sort_input(24, 4, 16, records, order))
    assert got[0] == "255"
    new = [int(x) for x in got[1].split()]
    assert new[:4] == order[:4] and new[20:] == order[20:]
    # longest first; equal durations in env order; negative records count as 0, that is last, among the zeros in env order
    assert new[4:20] == [5, 11, 17, 8, 9, 14, 10, 19, 4, 6, 15, 13, 18, 7, 12, 16]
    assert sorted(new[4:20]) == list(range(4, 20))


def test_sort_buckets_are_256_steps_of_the_longest_duration(policy):
    # kmax = 1000: bucket = duration * 255 // 1000 -- 999 and 998 share bucket 254 and keep env order, 1000 is alone in 255
    d = [998, 999, 1000, 3, 4, 0]       # 3 and 4: buckets 0 and 1; 3 shares bucket 0 with the idle env
    got = policy("sort", sort_input(6, 0, 6, [record(0, duration=x) for x in d], [9] * 6))
    assert got[0] == "1000" and [int(x) for x in got[1].split()] == [2, 0, 1, 4, 3, 5]


def test_sort_reports_that_no_env_reported_a_duration(policy):
    records = [[-1, -1, -1, -1]] * 5 + [record(0, ncon=3, duration=0)] * 3 + [record(0, duration=77)] * 2
    order = [7, 6, 5, 4, 3, 2, 1, 0, 8, 9]
    got = policy("sort", sort_input(10, 0, 8, records, order))      # (the envs with a duration are outside the range)
    assert got[0] == "0" and [int(x) for x in got[1].split()] == order   # left as it was: what then is the caller's


def tail_input(lo, records):
    return "%d %d %d\n%s\n" % (len(records), lo, len(records) - lo, " ".join(str(w) for r in records for w in r))


def test_tick_tail_ratio(policy):
    # 256 durations: 250 x 10, 3 x 50, 3 x 90.  p99 = sorted[256 - 1 - 256 // 100] = sorted[253] = 90; mean = 2920 / 256
    d = [10] * 250 + [50] * 3 + [90] * 3
    random.Random(5).shuffle(d)
    records = [record(0, ncon=17, duration=40000 // 2)] * 3 + [record(0, ncon=17, duration=x) for x in d]   # range starts at 3
    got = policy("tail", tail_input(3, records))
    assert abs(float(got[0]) - 90 * 256 / 2920) < 1e-5
    # envs that took no part are no samples: the same 256 among 44 absent ones
    mixed = records[3:] + [[-1, -1, -1, -1]] * 44
    random.Random(6).shuffle(mixed)
    assert abs(float(policy("tail", tail_input(0, mixed))[0]) - 90 * 256 / 2920) < 1e-5


def test_tick_tail_ratio_needs_256_samples(policy):
    assert policy("tail", tail_input(0, [record(0, duration=10 + i % 7) for i in range(255)])) == ["none"]
    # 300 envs of which 50 took no part
    records = [record(0, duration=20)] * 250 + [[-2, -1, -1, -1]] * 50
    assert policy("tail", tail_input(0, records)) == ["none"]
    assert policy("tail", tail_input(0, [record(0, duration=0)] * 256)) == ["none"]   # (nothing measured: no mean)


def test_free_staged_record(policy):
    cases = [(cur, ys) for cur in range(NSTAGE) for nout in range(1, RING + 1)
             for ys in itertools.product(range(NSTAGE), repeat=nout - 1)]     # the nout - 1 younger launches' records
    got = policy("free", "".join("%d %d %s\n" % (cur, len(ys), " ".join(map(str, ys))) for cur, ys in cases))
    assert len(got) == len(cases) == 5 * (1 + 5 + 25 + 125)
    for (cur, ys), g in zip(cases, got):
        pick = int(g)
        assert 0 <= pick < NSTAGE and pick != cur and pick not in ys, (cur, ys, pick)


def test_window_predicate(policy):
    # queue_min_ticks = 32, queue_tail_min = 1.45; tail: not measured / below / at / above
    tails = [(0, 0.0), (1, 1.2), (1, 1.45), (1, 1.9)]
    want = {7: [0, 0, 0, 0], 8: [1, 0, 1, 1], 31: [1, 0, 1, 1], 32: [1, 1, 1, 1], 200: [1, 1, 1, 1]}
    text = "".join("%d 32 %d %f 1.45\n" % (nt, v, t) for nt in want for v, t in tails)
    assert policy("window", text) == [str(x) for nt in want for x in want[nt]]
    # a stale tail (valid = 0) says nothing, however low
    assert policy("window", "8 32 0 1.0 1.45\n") == ["1"]


def test_ring_depth_kept_behind_a_launch(policy):
    # ring - 1 launches stay unprocessed behind a launch of up to 50 steps, none behind a longer one
    assert policy("keep", "1 2\n50 2\n51 2\n50 4\n2000 4\n5 3\n") == ["1", "1", "0", "3", "0", "2"]


def test_batch_must_exceed_the_wave_slots(policy):
    assert policy("fits", "1 2048 4096\n1 2048 2048\n1 2048 2049\n0 2048 4096\n1 0 4096\n") == ["1", "0", "1", "0", "0"]


def lwaves(policy, n, handovers, spare, wmax, envs):
    return int(policy("lwaves", "%d %d %d %d\n" % (n, handovers, spare, wmax) + "".join("%d %d %d\n" % e for e in envs))[0])


def test_queue_large_waves(policy):
    # 256 compute units: large_waves_max = 512, the balance is in units of 256 and never below 128
    # nothing flagged, nothing measured: r = 0, balance 0 -> floor 128; asked for: 0 + the 8 spare waves
    assert lwaves(policy, 4096, 0, 8, 512, [(-1, -1, 0)] * 4096) == 8
    # ... the last launch handed 20 envs over: 20 spare waves
    assert lwaves(policy, 4096, 20, 8, 512, [(-1, -1, 0)] * 4096) == 20
    # 1000 of 4096 flagged, every env 100 ticks: r = 1000 / 3096, x = 160 r / (26.5 r + 20.4) = 1.78457 per unit -> 456 waves
    envs = [(0, 100 << 16, 1)] * 1000 + [(0, 100 << 16, 0)] * 3096
    assert lwaves(policy, 4096, 0, 8, 512, envs) == int(160 * (1000 / 3096) / (26.5 * (1000 / 3096) + 20.4) * 256) == 456
    # the same without durations: a large tick counts as 1.3 compact ones, r = 1.3 * 1000 / 3096 -> x = 2.1299 -> 545
    envs = [(-1, -1, 1)] * 1000 + [(-1, -1, 0)] * 3096
    assert lwaves(policy, 4096, 0, 8, 512, envs) == 545
    # few large envs: a wave each and the spare ones, below the balance's floor of 128
    envs = [(0, 300 << 16, 1)] * 12 + [(0, 100 << 16, 0)] * 4084
    assert lwaves(policy, 4096, 0, 8, 512, envs) == 20
    # every env flagged: x -> 160 / 26.5 = 6.04 per unit (no compact work to balance against)
    assert lwaves(policy, 2000, 0, 8, 512, [(0, 100 << 16, 1)] * 2000) == int(160 / 26.5 * 256)
    # never zero
    assert lwaves(policy, 8, 0, 0, 0, [(-1, -1, 0)] * 8) == 1
