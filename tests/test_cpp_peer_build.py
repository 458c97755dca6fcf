"""CPU: the C++ ranks-as-processes layer without a GPU -- both one-sided drivers compile with plain g++ against the header-only host layer
(Shard::use_peer and the ABI's peer entries are declared), and the rendezvous of tests/cpp/process_ranks.hpp passes a 3-process run of
barriers, all-gathers and all-reduces; a rank that gives up makes the others leave promptly with their agreed exit code."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXIT_FAIL, EXIT_PEER_FAILED = 1, 5           # process_ranks::EXIT_FAIL / EXIT_PEER_FAILED


def _build(tmp, name, link=True):
    exe = os.path.join(str(tmp), name)
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe]
    if link:
        cmd += ["-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_peer_drivers_compile(tmp_path):
    assert os.path.exists(_build(tmp_path, "test_sw_sharded_peer"))
    assert os.path.exists(_build(tmp_path, "test_horiz_sharded_peer"))


def _run(exe, rdv, world, extra=()):
    procs = [subprocess.Popen(["timeout", "-k", "5", "60", exe, str(world), str(r), rdv, *extra], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    return [(p.wait(timeout=90), p.stdout.read()) for p in procs]


def test_rendezvous_three_processes(tmp_path):
    exe = _build(tmp_path, "test_process_ranks", link=False)
    rdv = str(tmp_path / "rendezvous")
    with open(rdv, "wb") as f:
        f.write(b"\0" * (1 << 20))
    res = _run(exe, rdv, 3)
    print(res)
    assert [rc for rc, _ in res] == [0, 0, 0] and all("DONE" in out for _, out in res)
    # a rank that gives up: the others leave their next wait at once instead of running into the 120 s limit
    with open(rdv, "wb") as f:
        f.write(b"\0" * (1 << 20))
    res = _run(exe, rdv, 3, ["fail"])
    print(res)
    assert [rc for rc, _ in res] == [EXIT_PEER_FAILED, EXIT_PEER_FAILED, EXIT_FAIL]
