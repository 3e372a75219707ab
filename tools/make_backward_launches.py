"""Write the launches per profile scope of one step of the cases of tests/test_gpu_backward_launches.py,
counted from the library loaded now:  python tools/make_backward_launches.py OUT.json COMMIT [case ...]   (GPU)

The committed tests/golden/backward_launches.json was written by this script with MARF_LIB set to a
build of the commit named in its "commit" field (its sources' hash in "source_hash"); the test compares
later builds against it.  Every case runs in a process of its own, as in make_step2_sched_bits.py."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "masking-bundle-adjusting-neural-radiance-fields_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def one(case):
    import step2_sched_cases as sc
    print(json.dumps(sc.case_launches(case, os.environ.__setitem__), sort_keys=True))


def main():
    import marf_hip
    import step2_sched_cases as sc
    out, commit = sys.argv[1], sys.argv[2]
    res = {"source_hash": marf_hip.lib().marf_source_hash().decode(), "commit": commit, "cases": {}}
    for c in sys.argv[3:] or sc.LAUNCH_CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", c], capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            raise SystemExit(f"{c}: exit {r.returncode}\n{r.stderr[-2000:]}")
        res["cases"][c] = json.loads(r.stdout.strip().splitlines()[-1])
        print(c, res["cases"][c], flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", out)


if __name__ == "__main__":
    if sys.argv[1] == "--case":
        one(sys.argv[2])
    else:
        main()
