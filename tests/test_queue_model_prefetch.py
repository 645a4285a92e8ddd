"""The queue launches' protocol with the early take, modelled on the CPU (tests/queue_model_prefetch/queue_model_prefetch.cpp:
threads for waves, the device code's lists, counters and order of atomic operations -- tests/test_queue_model.py models the
serial take).  A wave takes its next item in the middle of the current one, looks once more after it has listed its own
env when that found nothing, and keeps the item when the current tick is abandoned.  Checked by the model: the rows an
item was taken with are those of its tick, no wave takes the env it holds, every (env, tick) stepped exactly once and per
env in order, every thread terminates (no thread left waiting: the run ends, well inside its time limit), the finished
count exact.  Logic only, as in test_queue_model.py: memory ordering is covered on the device
(tests/test_gpu_queue_handoff.py).

And the rule for the waiting large launch's spare waves (csrc/mre_policy.h: queue_spare_large), values worked out from the
rule's text."""
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "queue_model_prefetch")


def _compile(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++17"] + flags + [os.path.join(HERE, name + ".cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return _compile(tmp_path_factory, "queue_model_prefetch", ["-O2", "-pthread"])


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    exe = _compile(tmp_path_factory, "spare_policy", ["-O1", "-Wall", "-Werror"])

    def run(mode, text):
        out = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (mode, out.stdout[-200:], out.stderr[-500:])
        return [int(x) for x in out.stdout.split()]
    return run


# N, T, waves, shards, large waves, overflow per mille, mode (0 side by side, 1 waiting large launch strictly first),
# early (bit 0: compact threads take early, bit 1: large threads do)
CASES = [
    (512, 24, 16, 4, 4, 10, 0, 3),
    (512, 24, 16, 4, 4, 10, 1, 3),      # hand-overs under both overlaps of the two kernels
    (40, 12, 64, 16, 2, 0, 0, 3),       # fewer envs than waves: most waves leave at once, every early take finds nothing
    (40, 12, 64, 16, 2, 50, 1, 3),
    (65, 12, 64, 16, 2, 0, 0, 3),       # envs = waves + 1: one env is always listed, whoever finishes first takes it
    (65, 12, 64, 16, 2, 50, 0, 3),
    (17, 20, 16, 4, 1, 100, 0, 3),      # the same with a tenth of the ticks abandoned, an item already taken
    (300, 16, 8, 3, 0, 30, 0, 3),       # no waiting large launch: the one behind the compact threads does everything
    (200, 6, 12, 4, 2, 1000, 0, 3),     # EVERY tick abandoned on the compact side
    (1024, 12, 24, 16, 1, 5, 0, 1),     # the large threads take serially
    (97, 20, 7, 5, 3, 20, 1, 0),        # nobody takes early (the PGS kernels): the protocol of test_queue_model.py
    (1, 8, 4, 2, 1, 0, 0, 3),           # one env: the wave that holds it finds nothing early, and the env again late
]


@pytest.mark.parametrize("case", CASES)
def test_every_tick_of_every_env_is_stepped_exactly_once_and_in_order(model, case):
    for seed in (1, 2, 3):
        out = subprocess.run([model] + [str(x) for x in case] + [str(seed)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.startswith("OK"), (case, seed, out.stdout, out.stderr)


def test_hand_overs_happen_in_the_model(model):
    out = subprocess.run([model] + [str(x) for x in (512, 24, 16, 4, 4, 10, 0, 3, 1)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert int(out.stdout.split()[-3]) > 0, out.stdout     # "... N handed over"


def test_spare_large_waves_by_need(policy):
    # the last launch handed nothing over: 1; it did: 8; MRE_QUEUE_SPARE_LARGE (forced >= 0) overrides both, 0 included
    assert policy("spare", "0 -1\n1 -1\n3 -1\n500 -1\n0 8\n0 0\n7 0\n7 32\n0 96\n") == [1, 8, 8, 8, 8, 0, 0, 32, 96]


def test_waiting_large_launch_with_spare_waves_by_need(policy):
    # 256 compute units: large_waves_max = 512; nothing measured, so the balance is at its floor of 128 throughout
    # (test_sched_policy.py: test_queue_large_waves) and the count is nl + max(last hand-overs, spare), at least 1
    rows = [
        ((4096, 0, 0, -1, 512), 1),      # nothing flagged, nothing handed over last time: the one spare wave
        ((4096, 0, 3, -1, 512), 8),      # 3 hand-overs last time: back to 8
        ((4096, 0, 20, -1, 512), 20),    # more hand-overs than that: as many
        ((4096, 12, 0, -1, 512), 13),    # a wave per large env and the one spare
        ((4096, 12, 2, -1, 512), 20),
        ((4096, 0, 0, 0, 512), 1),       # forced to none: never zero waves
        ((4096, 0, 5, 0, 512), 5),
        ((4096, 0, 0, 32, 512), 32),     # forced
        ((4096, 0, 0, 8, 512), 8),       # forced to the former default
    ]
    got = policy("lwaves", "".join("%d %d %d %d %d\n" % r[0] for r in rows))
    assert got == [r[1] for r in rows]
