#!/usr/bin/env python3
"""Is a refactor's device code the parent's? Compares, function by function, the gfx950 assembly and the resource
remarks of one set of compilation units against another's.

usage: tools/asm_compare.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...]
Each X.s comes from
    hipcc <the build's flags> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -o X.s X.hip 2> X.remarks
and X.remarks is read from beside it. A function's text is its instruction and local-label lines: comments, directives
and blank lines dropped, and the per-function index in local labels (.LBB<n>_<m>) blanked, since it counts the functions
in front of it in its unit. Prints one line per function of OLD (resources, line count, name; '!=' and both versions where NEW
differs) and exits 1 unless every function of OLD is defined exactly once across NEW with the same text and the same
resource line."""
import hashlib
import re
import sys

RES = (("VGPRs", "v"), ("VGPRs Spill", "vs"), ("TotalSGPRs", "s"), ("SGPRs Spill", "ss"), ("ScratchSize", "scr"),
       ("Occupancy", "occ"), ("LDS Size", "lds"))


def functions(path):
    """{name: [instruction lines]} of one assembly file."""
    out, cur, typed = {}, None, set()
    for line in open(path):
        line = line.split(";")[0].rstrip()
        m = re.match(r"^\s+\.type\s+([\w$.]+),@function$", line)
        if m:
            typed.add(m.group(1))
            continue
        m = re.match(r"^([\w$.]+):$", line)
        if m and m.group(1) in typed:
            assert m.group(1) not in out, (path, m.group(1))
            cur = out.setdefault(m.group(1), [])
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        s = line.strip()
        if cur is None or not s or (s.startswith(".") and not s.startswith(".L")):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", s)))
    return {k: v for k, v in out.items() if v}


def remarks(path):
    """{name: resource line} from the -Rpass-analysis=kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    for k, r in out.items():  # a remark this parser fails to read must not compare as equal
        assert all(key in r for key, _ in RES), (path, k, sorted(r))
    return {k: " ".join(f"{r[key]:>5} {tag}" for key, tag in RES) for k, r in out.items()}


def load(arg):
    fn, rs, dup = {}, {}, []
    for p in arg.split(","):
        unit = p.rsplit("/", 1)[-1]
        for k, v in functions(p).items():
            if k in fn:
                dup.append(k)
            fn[k] = (unit, v)
        rs.update(remarks(re.sub(r"\.s$", ".remarks", p)))
    return fn, rs, dup


def main():
    old, old_rs, _ = load(sys.argv[1])
    new, new_rs, dup = load(sys.argv[2])
    bad = 0
    for name in sorted(old, key=lambda n: (new.get(n, ("~",))[0], n)):
        unit, text = old[name]
        line = f"{old_rs.get(name, ''):<58} {len(text):>6} ins  {name}"
        if name not in new or name in dup:
            bad += 1
            print(f"!= {'defined twice' if name in dup else 'missing'}: {line}")
            continue
        nunit, ntext = new[name]
        same = ntext == text and new_rs.get(name) == old_rs.get(name)
        bad += not same
        print(f"{nunit}: {line}" if same else
              f"!= {nunit}: {line}\n   now: {new_rs.get(name, ''):<58} {len(ntext):>6} ins")
    extra = sorted(set(new) - set(old))
    for name in extra:
        print(f"!= only in NEW ({new[name][0]}): {name}")
    h = hashlib.sha256("\n".join(n + "\n" + "\n".join(old[n][1]) for n in sorted(old)).encode()).hexdigest()[:16]
    print(f"# {len(old)} functions in OLD, {len(new)} in NEW, {bad + len(extra)} differ; sha256 of OLD's text {h}")
    return 1 if bad or extra else 0


if __name__ == "__main__":
    sys.exit(main())
