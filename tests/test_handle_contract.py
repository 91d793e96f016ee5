"""The handle contract of include/po_hip.h (GPU): any entry may be called on one handle from several threads and each call is atomic; a handle's results do not depend on
what it solved before; distinct handles run side by side; a solve can be captured into a graph and replayed.  tools/handle_contract_check.py holds the scenarios (its
docstring lists them); every comparison there is BITWISE against the serial result of the same call on a fresh engine.

Each scenario runs in a child process of its own, one after the other, never two at once: a deadlock, an abort or a fault (what a broken contract can also look like)
costs one test and not the session — the reason tests/test_determinism.py gives for doing the same.  The timeouts stand beside the measured run times (one MI355X, wall
time of the child including the synthetic inputs and the serial references; 120 s leaves room for a cold start on a loaded machine, a deadlock still ends within it).
shared_handle_solve bites: against a library whose host-pointer entries release the lock between staging, launch and read-back (the state before the call lock of
po_capi.cpp) it printed DIFFER for all 8 thread checks — 14 to 20 of the 20 calls of every thread wrong, most of them bitwise equal to ANOTHER thread's serial result."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "handle_contract_check.py")

# scenario: (SAME lines it must print, timeout s, measured run time s)
SCENARIOS = {
    "shared_handle_solve": (10, 120, 3.2),   # 2 settings x (sizing call + 4 threads)
    "shared_handle_stages": (14, 120, 3.5),  # (4 sizing calls + 4 threads) + (3 + 3)
    "distinct_handles": (6, 120, 4.7),       # 6 threads
    "handle_reuse": (35, 120, 3.6),          # 3 parameter blocks x (9 calls + the repeat) + 4 smoothing calls + the repeat
    "graph_capture": (8, 120, 2.6),          # 2 settings x (warm-up + 3 replays)
}


def _run(name):
    n_lines, timeout, _ = SCENARIOS[name]
    r = subprocess.run([sys.executable, TOOL, name], capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("SAME", "DIFFER"))]
    print(r.stdout[-6000:])
    assert r.returncode == 0 and all(l.startswith("SAME ") for l in lines), (r.returncode, [l for l in lines if not l.startswith("SAME ")][:12], r.stdout[-1500:], r.stderr[-1500:])
    assert len(lines) == n_lines, (len(lines), r.stdout[-3000:])  # every check of the scenario ran


@pytest.mark.gpu
def test_four_threads_solving_on_one_handle_get_their_own_serial_results():
    _run("shared_handle_solve")


@pytest.mark.gpu
def test_threads_on_different_host_entries_of_one_handle_get_their_serial_results():
    _run("shared_handle_stages")


@pytest.mark.gpu
def test_six_handles_with_mixed_work_side_by_side_equal_serial():
    _run("distinct_handles")


@pytest.mark.gpu
def test_a_reused_handle_returns_what_a_fresh_one_returns():
    _run("handle_reuse")


@pytest.mark.gpu
def test_a_captured_solve_replays_bitwise_on_new_inputs():
    _run("graph_capture")


def test_the_tool_names_every_scenario_and_needs_no_gpu_to_import():
    r = subprocess.run([sys.executable, TOOL], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and all(name in r.stderr for name in SCENARIOS), r.stderr
