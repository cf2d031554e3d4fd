"""Compare the device code of two builds of libacmmp.so function by function (no GPU needed).

  python scripts/func_diff.py OLD.so NEW.so

Every gfx950 code object of each library is extracted (llvm-objdump --offloading) and disassembled (llvm-objdump -d);
a function's text is its instructions without addresses, encodings, branch-target symbols and the zero fill that
follows whichever function comes last in its section.  Names are demangled;
the last template argument of k_init, k_eval_ref and k_eval_ref_tail (PNEG) is written as a number on both sides (false
= 0, true = 1), since it changed type from bool to int.  Prints how many functions of OLD are in NEW with the same
text, the ones that differ or are missing, and the ones only NEW has."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
PNEG_KERNELS = ("acmmp::k_init<", "acmmp::k_eval_ref<", "acmmp::k_eval_ref_tail<")


def code_objects(lib, tmp):
    # llvm-objdump --offloading writes each bundle entry next to the file it reads: work on a copy
    work = os.path.join(tmp, str(len(os.listdir(tmp))))
    os.makedirs(work)
    copy = os.path.join(work, os.path.basename(lib))
    shutil.copy(lib, copy)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], capture_output=True, check=True)
    return sorted(os.path.join(work, f) for f in os.listdir(work) if "amdgcn" in f and f.endswith("gfx950"))


def norm_name(name):
    for k in PNEG_KERNELS:
        at = name.find(k)
        if at >= 0:
            name = re.sub(r", (true|false)>\(", lambda m: ", %d>(" % (m.group(1) == "true"), name, count=1)
    return name


def put(funcs, name, body):
    """A name defined in two code objects must have one text (it never overwrites another silently)."""
    text = "\n".join(body)
    if funcs.setdefault(name, text) != text:
        raise SystemExit(f"{name}: two definitions with different text in one library")


def functions(lib, tmp):
    funcs = {}
    for co in code_objects(lib, tmp):
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "-C", co],
                             capture_output=True, text=True, check=True).stdout
        name, body = None, []
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                if name:
                    put(funcs, name, body)
                name, body = norm_name(m.group(1)), []
                continue
            if name and line.strip():
                ins = line.split("//")[0].strip()
                ins = re.sub(r"<[^>]*>", "", ins).strip()
                if ins and ins != "...":       # (objdump's mark for the zero fill behind a section's last function)
                    body.append(ins)
        if name:
            put(funcs, name, body)
    return funcs


def main():
    old_lib, new_lib = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tmp:
        old, new = functions(old_lib, tmp), functions(new_lib, tmp)
    same = [n for n in old if new.get(n) == old[n]]
    differ = [n for n in old if n in new and new[n] != old[n]]
    missing = [n for n in old if n not in new]
    added = [n for n in new if n not in old]
    print(f"{len(old)} functions in {old_lib}, {len(new)} in {new_lib}")
    print(f"identical: {len(same)}; different text: {len(differ)}; missing: {len(missing)}; only in the new one: {len(added)}")
    for title, names in (("different", differ), ("missing", missing), ("added", added)):
        for n in sorted(names):
            print(f"  {title}: {n}")
    return 0 if not differ and not missing else 1


if __name__ == "__main__":
    sys.exit(main())
