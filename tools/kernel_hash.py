#!/usr/bin/env python3
"""Hash the device code of every kernel of csrc/, to show that a move of source text changed no instruction.

  kernel_hash.py emit CSRC_DIR OUT.json [SUFFIX]
                                            compile every .hip unit of CSRC_DIR to gfx950 assembly with the flags its Makefile
                                            gives the unit's object, hash every function body -> {symbol: [unit, sha256]}.
                                            With SUFFIX (_literal, _latestage, _texp1): the objects of libaadffSUFFIX.so, i.e.
                                            UNIT_SUFFIX.o for the units that library builds as a variant and UNIT.o for the rest
  kernel_hash.py compare OLD.json NEW.json  markdown table: symbol, old hash, new hash, same / different / only in one

A body is the text between the symbol's label and its .Lfunc_end, plus its .amdhsa_kernel descriptor (registers, LDS), with
comments stripped and the compiler's local label numbers (.LBBn_m, .Ltmpn, which count functions and labels of the whole unit)
normalised.  A symbol's own mangled name inside its body (function-local LDS arrays carry it) is replaced by a placeholder, so
that a kernel whose parameter type moved to another namespace can still be matched by its body.  Only hashes are written.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile


def unit_asm(csrc, unit, tmp):
    """assembly of one object (a unit's name, with the variant's suffix if any): the Makefile's own compile command for unit.o,
    turned into a device-only -S run"""
    cmd = subprocess.check_output(["make", "-C", csrc, "-n", "-B", "--no-print-directory", unit + ".o"], text=True).strip().splitlines()
    cmd = [c for c in cmd if " -c " in c and c.rstrip().endswith(unit + ".o")][-1].split()
    out = os.path.join(tmp, unit + ".s")
    cmd = cmd[:cmd.index("-o")] + ["-o", out]
    cmd[cmd.index("-c")] = "-S"
    subprocess.check_call(cmd + ["--cuda-device-only"], cwd=csrc)
    with open(out) as f:
        return f.read()


def normalise(lines, sym):
    tmp_ids = {}
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip():
            continue
        ln = ln.replace(sym[2:], "<self>")
        ln = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", ln)
        ln = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", ln)
        ln = re.sub(r"\.Ltmp(\d+)", lambda m: ".Ltmp%d" % tmp_ids.setdefault(m.group(1), len(tmp_ids)), ln)
        out.append(ln)
    return "\n".join(out)


def bodies(asm):
    lines = asm.splitlines()
    funcs = [m.group(1) for ln in lines for m in [re.match(r"\s*\.type\s+(\S+),@function", ln)] if m]
    res = {}
    for sym in funcs:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        text = lines[start + 1:end]
        head = "\t.amdhsa_kernel " + sym
        if head in lines:
            k0 = lines.index(head)
            k1 = next(i for i in range(k0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
            text = text + lines[k0 + 1:k1]
        res[sym] = hashlib.sha256(normalise(text, sym).encode()).hexdigest()
    return res


def emit(csrc, out, suffix=""):
    table = {}
    variant = set()
    if suffix:                                # the objects on the link line of the variant's library
        link = subprocess.check_output(["make", "-C", csrc, "-n", "-B", "--no-print-directory", f"libaadff{suffix}.so"], text=True)
        variant = {w for ln in link.splitlines() if " -shared " in ln for w in ln.split() if w.endswith(suffix + ".o")}
    with tempfile.TemporaryDirectory() as tmp:
        for src in sorted(os.listdir(csrc)):
            if src.endswith(".hip"):
                obj = src[:-4] + suffix if src[:-4] + suffix + ".o" in variant else src[:-4]
                for sym, h in bodies(unit_asm(csrc, obj, tmp)).items():
                    table[sym] = [src, h]
    with open(out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
    print(f"{len(table)} functions of {csrc} -> {out}")


def demangle(syms):
    out = subprocess.run(["c++filt"], input="\n".join(syms), text=True, capture_output=True).stdout.splitlines()
    return dict(zip(syms, out))


def compare(old_path, new_path):
    old, new = json.load(open(old_path)), json.load(open(new_path))
    names = demangle(sorted(set(old) | set(new)))
    base = lambda s: re.sub(r"<.*", "", names[s].replace("void ", "").split("(")[0]).split("::")[-1]
    only_new = {s for s in new if s not in old}
    rows, n_same, n_diff = [], 0, 0
    for s in sorted(set(old) | set(new), key=lambda s: (names[s], s)):
        if s in old and s in new:
            same = old[s][1] == new[s][1]
            n_same += same
            n_diff += not same
            rows.append((names[s], old[s][0], old[s][1][:16], new[s][0], new[s][1][:16], "same" if same else "DIFFERENT"))
        elif s in old:
            # a symbol whose name changed (a parameter type moved to another namespace): match it by function name and body
            twin = [t for t in only_new if base(t) == base(s) and new[t][1] == old[s][1]]
            if len(twin) == 1:
                n_same += 1
                rows.append((names[s], old[s][0], old[s][1][:16], new[twin[0]][0], new[twin[0]][1][:16], "same body, renamed to " + names[twin[0]]))
                only_new.discard(twin[0])
            else:
                rows.append((names[s], old[s][0], old[s][1][:16], "-", "-", "only in old"))
    for s in sorted(only_new, key=lambda s: names[s]):
        rows.append((names[s], "-", "-", new[s][0], new[s][1][:16], "only in new"))
    print("| function | old unit | old sha256[:16] | new unit | new sha256[:16] | result |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| `" + r[0].replace("|", "\\|") + "` | " + " | ".join(r[1:]) + " |")
    print(f"\n{n_same} same, {n_diff} different, {sum(r[5] == 'only in old' for r in rows)} only in old, "
          f"{sum(r[5] == 'only in new' for r in rows)} only in new.")


if __name__ == "__main__":
    if len(sys.argv) in (4, 5) and sys.argv[1] == "emit":
        emit(*sys.argv[2:])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
