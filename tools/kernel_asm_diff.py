"""Compare the device code of two builds of one translation unit, kernel by kernel.

    hipcc ... --cuda-device-only -S -o a.s x.hip     (once per tree)
    python tools/kernel_asm_diff.py a.s b.s [--grown]

Prints, per kernel symbol (demangled with c++filt when it is on the PATH), whether the instruction stream between the
symbol's label and its .Lfunc_end is identical in the two files, and lists the kernels only one of them has.  The
function's ordinal in the file, which clang writes into its block labels and loop comments (BB<ordinal>_<block>), is dropped -- a
kernel added before it shifts it -- and nothing else: a kernel that is reported identical is so line for line.
--grown: a template kernel of a.s without a namesake in b.s is compared with b.s's instantiation that has the same
leading template arguments and one more, `false` (a switch added with its default off, which changes the mangled name
and may add trailing kernel arguments); lines that hold either mangled name are skipped and the differing lines are
printed -- the kernel descriptor's .amdhsa_kernarg_size is the one to expect.
Exit status 1 when a kernel both files have differs.
"""
import re
import shutil
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if name is None and m and not line.startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(re.sub(r"\bBB\d+_|\.LBB\d+_", lambda m: re.sub(r"\d+", "", m.group(0)), line.rstrip()))
    return out


def demangle(names):
    if not names or shutil.which("c++filt") is None:
        return {n: n for n in names}
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, res.stdout.splitlines()))


def grown_match(name, names, kb):
    """b's kernel whose demangled name is `name` with one more template argument, false."""
    head, sep, tail = name.partition(">(")
    for n in kb:
        if names[n].startswith(head + ", false>("):
            return n
    return None


def main(a, b, grown=False):
    ka, kb = kernels(a), kernels(b)
    names = demangle(sorted(set(ka) | set(kb)))
    bad = 0
    paired = set()
    for n in sorted(names, key=names.get):
        if n in ka and n in kb:
            same = ka[n] == kb[n]
            bad += not same
            print(f"{'identical' if same else 'DIFFERENT':10s} {len(ka[n]):6d} lines  {names[n]}")
            continue
        m = grown_match(names[n], names, kb) if (grown and n in ka) else None
        if m is not None:
            paired.add(m)
            la = [x for x in ka[n] if n not in x]
            lb = [x for x in kb[m] if m not in x]
            diff = [(x.strip(), y.strip()) for x, y in zip(la, lb) if x != y] if len(la) == len(lb) else None
            print(f"{'grown':10s} {len(la):6d} lines  {names[n].split('(')[0]}: " +
                  ("line counts differ" if diff is None else f"differing lines {diff}"))
            bad += diff is None or any("kernarg_size" not in x for x, _ in diff)
        elif n not in paired:
            print(f"{'only in ' + (a if n in ka else b)}  {names[n]}")
    return 1 if bad else 0


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "--grown"]
    sys.exit(main(args[0], args[1], grown="--grown" in sys.argv))
