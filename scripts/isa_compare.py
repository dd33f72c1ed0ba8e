#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel (no GPU): instructions and the compiler's resource lines.

    hipcc <the Makefile's flags> -x hip --cuda-device-only -S -fuse-cuid=none FILE.hip -o parent_FILE.s     (at the parent commit)
    hipcc ...                                                                         -o tree_FILE.s       (in the tree)
    python scripts/isa_compare.py --focus k_prep,k_guide_march,k_chunk_min parent_FILE.s tree_FILE.s [more pairs ...]

Every kernel of the tree is matched with the parent's kernel of the same demangled name; a focus kernel whose signature changed is
matched with the parent's kernel of the same name and template head (its "role": the leading non-type template arguments), a
k_cvf_pc instantiation with the parent's of the same form and source (pair_key).  Per kernel: VGPRs, SGPRs, scratch, LDS,
occupancy, the memory instructions by address space, and a verdict - identical / same sequence / same vector+memory+LDS multiset /
DIFFERS with the counts that changed."""
import argparse
import collections
import re
import subprocess


def kernels(path):
    """name -> (instruction lines, resources) of every kernel of an assembly file"""
    out, name, body = {}, None, []
    res = {}
    text = open(path).read().split("\n")
    for ln in text:
        m = re.match(r"^(_Z\w+|k_\w+):\s*(;.*)?$", ln)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            m = re.match(r"^; (NumVgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", ln)
            if m and res.get("_last"):
                out[res["_last"]][1][m.group(1)] = int(m.group(2))
            continue
        s = ln.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            out[name] = (body, {})
            res["_last"] = name
            name = None
            continue
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))      # (branch targets carry the function's number in the file)
    return {k: v for k, v in out.items() if v[1]}


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.split("\n")))


def mnem(lines):
    return [ln.split()[0] for ln in lines]


def is_scalar(m):
    return m.startswith("s_")


def mem_mix(lines):
    c = collections.Counter()
    for m in mnem(lines):
        for p in ("flat_", "global_", "buffer_", "scratch_", "ds_"):
            if m.startswith(p):
                c[p.rstrip("_")] += 1
    return c


def verdict(a, b):
    if a == b:
        return "identical"
    ma, mb = mnem(a), mnem(b)
    if ma == mb:
        return "same instruction sequence, operands differ (registers / kernarg offsets)"
    ca = collections.Counter(m for m in ma if not is_scalar(m))
    cb = collections.Counter(m for m in mb if not is_scalar(m))
    same = ca == cb
    ca, cb = collections.Counter(ma), collections.Counter(mb)
    d = ", ".join("%s %d -> %d" % (k, ca[k], cb[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k])
    if same:
        return "same VALU/memory/LDS instruction multiset; scalar set-up / order differs (%d -> %d instr)%s" % (len(a), len(b), ": " + d if d else "")
    return "DIFFERS (%d -> %d instr): %s" % (len(a), len(b), d)


def template_head(dem):
    """(kernel name, its template arguments) of a demangled name"""
    m = re.match(r"^(?:void )?(?:psm::)?(\w+)(?:<([^()]*?)>)?\(", dem)
    if not m:
        return dem, []
    return m.group(1), [a.strip() for a in re.split(r",\s*(?![^<]*>)", m.group(2) or "") if a.strip()]


def role(dem):
    """name + leading non-type template arguments: k_prep<true, ...> -> k_prep<true>"""
    name, args = template_head(dem)
    lead = []
    for a in args:
        if re.match(r"^(true|false|\(?\w*\)?-?\d+)$", a):
            lead.append(a)
        else:
            break
    return name + ("<" + ", ".join(lead) + ">" if lead else "")


def pair_key(dem):
    """What pairs a tree kernel with the parent's across a signature change: its role - and for k_cvf_pc the whole instantiation,
    whose record source S took the place of a flag further back: <VEC4, CVC, MODE, U8, BATCH, VAR, NARROW> with BATCH = false is
    <VEC4, CVC, MODE, S, U8, VAR, NARROW> over the pair by value, BATCH = true the one over the table."""
    name, args = template_head(dem)
    if name != "k_cvf_pc" or len(args) != 7:
        return role(dem)
    if source_of(dem):
        v4, cvc, mode, _, u8, var, narrow = args
        src = source_of(dem)
    else:
        v4, cvc, mode, u8, batch, var, narrow = args
        src = "table" if batch == "true" else "value"
    return "k_cvf_pc<%s> [%s]" % (", ".join((v4, cvc, mode, u8, var, narrow)), src)


def source_of(dem):
    if "RecVal<" in dem:
        return "value"
    if re.search(r"<[^()]*const\*[^()]*>\(", dem) or re.search(r"PcPair const\*>", dem):
        return "table"
    return ""


def line(r, mix):
    return "vgpr %d sgpr %d scratch %d lds %d occ %d | %s" % (
        r["NumVgprs"], r["TotalNumSgprs"], r["ScratchSize"], r["LDSByteSize"], r["Occupancy"],
        " ".join("%s %d" % kv for kv in sorted(mix.items())) or "no memory instruction")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--focus", default="", help="comma-separated kernel names matched by role when the signature changed")
    ap.add_argument("files", nargs="+", help="parent.s tree.s [parent2.s tree2.s ...]")
    a = ap.parse_args()
    focus = [f for f in a.focus.split(",") if f]
    counts = collections.Counter()
    for pf, tf in zip(a.files[0::2], a.files[1::2]):
        P, T = kernels(pf), kernels(tf)
        dp, dt = demangle(list(P)), demangle(list(T))
        print("== %s -> %s: %d -> %d kernels ==" % (pf.split("/")[-1], tf.split("/")[-1], len(P), len(T)))
        by_role = collections.defaultdict(list)
        for n in P:
            by_role[pair_key(dp[n])].append(n)
        gone = set(P) - set(T)
        for n in sorted(T, key=lambda k: dt[k]):
            short = re.sub(r"^void ", "", dt[n]).split("(")[0]
            if n in P:
                v = verdict(P[n][0], T[n][0])
                chg = ["%s %d -> %d" % (k, P[n][1][k], T[n][1][k]) for k in sorted(T[n][1]) if P[n][1].get(k) != T[n][1][k]]
                counts[v.split(" (")[0].split(";")[0]] += 1
                if v != "identical" or chg:
                    print(short)
                    print("    " + line(T[n][1], mem_mix(T[n][0])))
                    print("    " + v + ("".join(" | " + c for c in chg)))
                continue
            r, key = role(dt[n]), pair_key(dt[n])
            if not any(r == f or r.startswith(f + "<") for f in focus) or key not in by_role:
                print(short)
                print("    " + line(T[n][1], mem_mix(T[n][0])))
                print("    NEW: no kernel of this name in the parent")
                counts["new"] += 1
                continue
            for pn in by_role[key]:
                gone.discard(pn)
                print("%s   against the parent's %s" % (key if key != r else "%s [%s]" % (r, source_of(dt[n])),
                                                        re.sub(r"^void (psm::)?", "", dp[pn]).split("(")[0] if key != r else role(dp[pn])))
                print("    parent: " + line(P[pn][1], mem_mix(P[pn][0])))
                print("    tree:   " + line(T[n][1], mem_mix(T[n][0])))
                chg = ["%s %d -> %d" % (k, P[pn][1][k], T[n][1][k]) for k in sorted(T[n][1]) if P[pn][1].get(k) != T[n][1][k]]
                print("    " + verdict(P[pn][0], T[n][0]) + "".join(" | " + c for c in chg))
                counts["focus"] += 1
        for n in sorted(gone):
            print("GONE: " + re.sub(r"^void ", "", dp[n]).split("(")[0])
    print("summary: " + ", ".join("%d %s" % (v, k) for k, v in counts.most_common()))


if __name__ == "__main__":
    main()
