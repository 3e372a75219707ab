"""Static instruction census of the step kernel's hot regions in a hipcc -S listing.

    python tools/isa_census.py <file.s> [mangled kernel name]
    python tools/isa_census.py --stores <file.s> [mangled kernel name]   (the kernel's vector global stores by opcode)

(default kernel: k_step2<256, true, 4, 4, 5, 3>, the instantiation bench.py runs).  Three regions,
found from the control flow and the MFMA shapes alone:

  hidden forward loop   the first innermost loop with >= 100 v_mfma_f32_32x32x16 instructions
  hidden dgrad loop     the second such loop
  dW_last block         from the start of the basic block with the first v_mfma_f32_16x16x32 to the
                        next s_barrier or v_mfma_f32_32x32x16 after the last one

For each it prints the MFMA count, the other VALU by opcode, the three register-copy opcodes
(v_accvgpr_read / v_accvgpr_write / v_mov_b32), SALU split into s_nop / s_waitcnt / the rest, DS
and vector-memory counts, and all of them per MFMA.  Instructions are classified by opcode prefix;
the only operand it looks at is the lgkmcnt(0) of an s_waitcnt (the full LDS drains)."""
import re
import sys
from collections import Counter

FLAGSHIP = "_ZN4marf7k_step2ILi256ELb1ELi4ELi4ELi5ELi3EEEvNS_9Step2ArgsE"
COPIES = ("v_accvgpr_read", "v_accvgpr_write", "v_mov_b32")


def kernel_lines(path, name):
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    out = []
    for l in lines[start + 1:]:
        t = l.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            break
        if t and (not t.startswith(".") or re.match(r"^\.LBB\w+:", t)):
            out.append(t)
    return out


def census(ins):
    c = {"mfma": 0, "valu": Counter(), "copy": Counter(), "s_nop": 0, "s_waitcnt": 0, "drain": 0, "salu": 0, "ds": 0,
         "vmem": 0}
    for t in ins:
        op = t.split()[0]
        if op.endswith(":"):
            continue
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith(COPIES):
            c["copy"][next(k for k in COPIES if op.startswith(k))] += 1
        elif op.startswith("v_"):
            c["valu"][op] += 1
        elif op.startswith("ds_"):
            c["ds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("s_nop"):
            c["s_nop"] += 1
        elif op.startswith("s_waitcnt"):
            c["s_waitcnt"] += 1
            if "lgkmcnt(0)" in t:
                c["drain"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    return c


def report(title, ins):
    c = census(ins)
    m = max(c["mfma"], 1)
    nv, nc = sum(c["valu"].values()), sum(c["copy"].values())
    ns = c["s_nop"] + c["s_waitcnt"] + c["salu"]
    print(f"== {title}: {len(ins)} lines, {c['mfma']} MFMA")
    print(f"   VALU (no copies) {nv} = {nv / m:.2f} per MFMA: " + ", ".join(f"{k} {v}" for k, v in c["valu"].most_common()))
    print(f"   copies {nc} = {nc / m:.2f} per MFMA: " + " / ".join(f"{k} {c['copy'][k]}" for k in COPIES))
    print(f"   SALU {ns} = {ns / m:.2f} per MFMA: s_nop {c['s_nop']}, s_waitcnt {c['s_waitcnt']} "
          f"(lgkmcnt(0) drains {c['drain']}), other {c['salu']}")
    print(f"   DS {c['ds']} = {c['ds'] / m:.2f} per MFMA, VMEM {c['vmem']} = {c['vmem'] / m:.2f} per MFMA")
    tot = nv + nc + ns + c["ds"] + c["vmem"]
    print(f"   non-MFMA per MFMA {tot / m:.2f}")


def stores(ins):
    """Vector global stores of a whole kernel, by opcode (static count: an instruction in a loop is one)."""
    c = Counter(t.split()[0] for t in ins if t.startswith(("global_store", "global_atomic", "buffer_store", "flat_store",
                                                           "scratch_store")))
    return c


def main():
    args = [a for a in sys.argv[1:] if a != "--stores"]
    path = args[0]
    name = args[1] if len(args) > 1 else FLAGSHIP
    ins = kernel_lines(path, name)
    if "--stores" in sys.argv:  # python tools/isa_census.py --stores <file.s> [kernel]: the store census alone
        c = stores(ins)
        print(f"== {name}: {sum(c.values())} vector global store instructions: " +
              (", ".join(f"{k} {v}" for k, v in sorted(c.items())) or "none"))
        return
    label = {t[:-1]: i for i, t in enumerate(ins) if t.endswith(":")}
    big = [i for i, t in enumerate(ins) if t.startswith("v_mfma_f32_32x32x16")]
    loops = []
    for i, t in enumerate(ins):
        if t.startswith(("s_cbranch", "s_branch")):
            tgt = label.get(t.split()[-1])
            if tgt is not None and tgt <= i and sum(tgt <= b <= i for b in big) >= 100:
                loops.append((tgt, i))
    inner = sorted(l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops))
    for title, l in zip(("hidden forward loop", "hidden dgrad loop"), inner):
        report(title, ins[l[0]:l[1] + 1])
    small = [i for i, t in enumerate(ins) if t.startswith("v_mfma_f32_16x16x32")]
    if small:
        s = max(i for i in label.values() if i <= small[0])
        e = next((i for i in range(small[-1] + 1, len(ins)) if ins[i].startswith(("s_barrier", "v_mfma_f32_32x32x16"))),
                 len(ins))
        report("dW_last block", ins[s:e])


if __name__ == "__main__":
    main()
