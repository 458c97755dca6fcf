"""The C++ hosts of the two Strang steps against the Python hosts at the same commit, on one GPU:

  box           config-5 grid (p = 4, 32 x 32 box, 64 levels, dt = 0.01, do_visc off, 3 Newton iterations): mimsem_amd/host/euler_call on the case
                scripts/run_bubble.py --write-case wrote (mimsem_host::box::Euler) against scripts/run_bubble.py (BoxEuler.strang)
  held-suarez   scripts/run_umjs14.py --case held-suarez (p = 3, 24 x 24 x 6 sphere, 16 levels, dt = 120): euler_call --integrator strang
                (mimsem_host::eul::Euler::Strang) against the script itself (Euler.strang)

Every run is a process of its own with its own warm-up (Python: one step, C++: two) and reports the median of its timed steps, host clock
around a step that ends in the read of the energetics line; REPEATS runs per host, the hosts alternating; the median, minimum and maximum
of those run medians are written.  Writes profiles/cpp_steps.txt (or the path given)."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS, STEPS = 3, 6
CASES = {"box": (["scripts/run_bubble.py", "--pn", "4", "--ne", "32", "--nk", "64", "--dt", "0.01", "--newton-maxit", "3"], []),
         "held-suarez": (["scripts/run_umjs14.py", "--case", "held-suarez"], ["--integrator", "strang"])}


def run(cmd, timeout=600):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise SystemExit("%s failed (%d):\n%s\n%s" % (" ".join(cmd), p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
    return p.stdout


def python_host(driver, tmp):
    out = run([sys.executable] + driver + ["--nsteps", str(STEPS + 1), "--outdir", os.path.join(tmp, "out")])
    m = re.search(r"median ([0-9.]+), min ([0-9.]+), max ([0-9.]+)", out)
    n = re.search(r"Newton iterations per step[^:]*: ([0-9 ]+)", out)
    return float(m.group(1)), (n.group(1).split() if n else [])


def cpp_host(case, extra):
    j = json.loads(run([os.path.join(ROOT, "mimsem_amd", "host", "euler_call"), case, str(STEPS), "2"] + extra).strip().splitlines()[-1])
    return j["ms_per_step_median"], j


def main(path):
    lines = ["C++ hosts of Euler::Strang and the box step against the Python hosts; %d runs per host, alternating, each a process with its own warm-up,"
             % REPEATS, "the median of %d timed steps per run (host clock, diagnostics on); median (min .. max) of the run medians in ms" % STEPS, ""]
    with tempfile.TemporaryDirectory() as tmp:
        for name, (driver, extra) in CASES.items():
            case = os.path.join(tmp, name + ".case")
            run([sys.executable] + driver + ["--nsteps", str(STEPS), "--write-case", case])
            py, cpp, info, newton = [], [], None, []
            for _ in range(REPEATS):
                t, newton = python_host(driver, tmp)
                py.append(t)
                t, info = cpp_host(case, extra)
                cpp.append(t)
            fmt = lambda v: "%.2f (%.2f .. %.2f)" % (np.median(v), min(v), max(v))
            lines += ["%-12s Python host %s   C++ host %s   C++ / Python (medians) %.3f" % (name, fmt(py), fmt(cpp), np.median(cpp) / np.median(py)),
                      "             C++: %s, %d elements, order %d, %d levels, Newton iterations per step %.2f, steps redone %d, state finite %s; Python: Newton %s"
                      % (info["integrator"], info["elements"], info["order"], info["levels"], info["newton_per_step"], info["redone"], info["finite"],
                         " ".join(newton))]
            print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cpp_steps.txt"))
