"""Dev tool (CPU): fp64 opcode totals of whole assembly listings (`hipcc -S --cuda-device-only`), grouped the way DESIGN.md section 19 quotes them — add, mul, fused
(v_fma_f64 + v_fmac_f64: two encodings of one operation), min / max, compares, v_rcp, v_div_* — so that two builds can be compared for moved contraction: a changed mul,
add or fused total means a multiply and an add were fused somewhere else.      python tools/fp64_opcode_totals.py a.s [b.s ...]"""
import collections, re, sys

GROUPS = (("add", r"v_add_f64"), ("mul", r"v_mul_f64"), ("fma", r"v_fma_f64"), ("fmac", r"v_fmac_f64"), ("max", r"v_max_f64"), ("min", r"v_min_f64"), ("cmp", r"v_cmpx?_\w+_f64"),
          ("rcp", r"v_rcp_f64"), ("div_scale", r"v_div_scale_f64"), ("div_fmas", r"v_div_fmas_f64"), ("div_fixup", r"v_div_fixup_f64"), ("other_f64", r"v_\w*f64\w*"))


def totals(path):
    c = collections.Counter()
    n = scratch = lane = 0
    for l in open(path):
        if not l.startswith("\t") or l.startswith("\t.") or l.startswith("\t;"):
            continue
        op = l.split()[0]
        n += 1
        scratch += op.startswith("scratch_")
        lane += op.startswith(("v_readlane", "v_writelane", "v_readfirstlane"))
        for g, rx in GROUPS:
            if re.fullmatch(rx + r"(_e32|_e64|_dpp|_sdwa)?", op):
                c[g] += 1
                break
    c["fused"] = c["fma"] + c["fmac"]
    return n, scratch, lane, c


if __name__ == "__main__":
    for p in sys.argv[1:]:
        n, scratch, lane, c = totals(p)
        print(f"{p}: instructions {n}, scratch {scratch}, lane moves {lane}; fp64: " + " ".join(f"{g} {c[g]}" for g in ("add", "mul", "fused", "fma", "fmac", "max", "min", "cmp", "rcp", "div_scale", "div_fmas", "div_fixup", "other_f64")))
