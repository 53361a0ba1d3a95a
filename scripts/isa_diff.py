#!/usr/bin/env python3
"""Are two builds of the device code the same?  usage: isa_diff.py OLD.s NEW.s

Both inputs are `hipcc --cuda-device-only -S` outputs of csrc/nvllm.hip (the flags are in scripts/check_isa.sh).  Compares,
by mangled name, every function's body (instructions, directives and the kernel descriptor that follows it) and every
kernel's entry in the code object metadata (registers, spills, LDS, scratch, kernarg layout).  Comments and blank lines
are dropped and local labels (.LBB12_3, .Lfunc_end12, ...) are renumbered in order of appearance, so moving a function
inside the file changes nothing.  Prints the added, removed and changed symbols; exit status 1 on any difference.
It compares the two files and nothing else: what the kernels must look like is scripts/check_isa.sh's business."""
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z_$][\w$.]*")
META_KEYS = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
             "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")


def functions(text):
    """{mangled name: normalised body lines} for every `.type NAME,@function` ... `.Lfunc_endN:` span"""
    out, name, body, labels = {}, None, [], {}
    for raw in text.split("\n"):
        m = re.match(r"\s*\.type\s+(\S+),@function", raw)
        if m:
            name, body, labels = m.group(1), [], {}
            continue
        if name is None:
            continue
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        line = LABEL.sub(lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), line)
        body.append(" ".join(line.split()))
        if raw.startswith(".Lfunc_end"):
            out[name], name = body, None
    return out


def metadata(text):
    """{kernel name: normalised lines of its amdhsa.kernels entry}"""
    m = re.search(r"\n\s*\.amdgpu_metadata\n(.*?)\n\s*\.end_amdgpu_metadata", text, re.S)
    out = {}
    if m:
        for entry in re.split(r"\n  - (?=\.)", m.group(1).split("amdhsa.kernels:", 1)[1])[1:]:
            lines = [" ".join(l.split()) for l in entry.split("\n") if l.strip() and not l.startswith("amdhsa.")]
            name = next(l.split(None, 1)[1] for l in lines if l.startswith(".name:"))
            out[name] = lines
    return out


def report(what, old, new, detail):
    added, removed = sorted(set(new) - set(old)), sorted(set(old) - set(new))
    changed = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    print("%s: %d old, %d new, %d added, %d removed, %d changed" % (what, len(old), len(new), len(added), len(removed), len(changed)))
    for tag, names in (("added", added), ("removed", removed)):
        for k in names:
            print("  %-8s %s" % (tag, k))
    for k in changed:
        print("  %-8s %s  %s" % ("changed", k, detail(old[k], new[k])))
    return len(added) + len(removed) + len(changed)


def body_detail(a, b):
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return "(%d -> %d lines, first difference at line %d)" % (len(a), len(b), first + 1)


def meta_detail(a, b):
    val = lambda lines, key: next((l.split(":", 1)[1].strip() for l in lines if l.startswith("." + key + ":")), "?")
    diffs = ["%s %s -> %s" % (k, val(a, k), val(b, k)) for k in META_KEYS if val(a, k) != val(b, k)]
    return "(" + (", ".join(diffs) or "arguments") + ")"


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = (open(p).read() for p in sys.argv[1:])
    bad = report("functions", functions(old), functions(new), body_detail)
    bad += report("kernel metadata", metadata(old), metadata(new), meta_detail)
    print("device code differs" if bad else "device code identical")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
