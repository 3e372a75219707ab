"""Write the host buffer-plan figures (tests/plan_bytes_cases.py) given by the library loaded now:
python tools/make_plan_bytes.py OUT.json   (no GPU needed: planning reads no device memory)

The committed tests/golden/plan_bytes.json was written by this script from the library named in its
"source_hash" / "commit" fields; test_plan_bytes_cpu.py compares later builds against it."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "masking-bundle-adjusting-neural-radiance-fields_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    import marf_hip
    import plan_bytes_cases
    out = sys.argv[1]
    try:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"source_hash": marf_hip.lib().marf_source_hash().decode(), "commit": commit or None}
    res.update(plan_bytes_cases.record())
    for k, v in res["nets"].items():
        print(k, v["step_kernel"], v["geometries"]["3x16x20"]["step_saved_bytes"], flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", out)


if __name__ == "__main__":
    main()
