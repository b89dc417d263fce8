"""What the gfx950 code object says of each kernel: the AMDGPU metadata note
(llvm-readelf --notes) of the device ELF inside build/obj/md5_kernels.o or
libmd5hip.so, by kernel name as the launch records spell it
("md5hip::md5_desc_fed<true>").  Metadata only: nothing is disassembled.
Test infrastructure.

(after `make -C tests/c launch_check`, which names the kernels)
    python tests/kernel_resources.py            # the table, as JSON
    python tests/kernel_resources.py --write    # tests/golden/kernel_resources.json

The golden file holds the VGPR and SGPR-spill counts of the commit it was
written at, with the compiler's version string: tests/test_launch_routes.py
lets neither grow while the compiler is the same."""
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
OBJECT = os.path.join(REPO, "build", "obj", "md5_kernels.o")
GOLDEN = os.path.join(REPO, "tests", "golden", "kernel_resources.json")
FIELDS = ("agpr_count", "vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
          "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size")


def compiler_version() -> str:
    """hipcc's HIP version and its clang's version line"""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    out = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True)
    return "; ".join(line.strip() for line in out.stdout.splitlines()[:2])


def read(names: dict, path: str = OBJECT) -> dict:
    """{kernel: {field: int}} for the kernels of the code object in `path` that
    `names` ({mangled: name}, from `launch_check --kernels`) lists."""
    sys.path.insert(0, REPO)
    from sproxy_amd import _lib
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(_lib._device_elf(path))
        f.flush()
        notes = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", f.name],
                               capture_output=True, text=True, check=True).stdout
    kernels, cur = [], None
    for line in notes.splitlines():
        m = re.match(r"\s+(- )?\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        dash, key, val = m.groups()
        # a kernel's map starts with its first key, .agpr_count, behind a dash at the kernels' depth
        if dash and key == "agpr_count":
            cur = {}
            kernels.append(cur)
        if cur is not None and (key in FIELDS or key == "name") and key not in cur:
            cur[key] = val
    out = {}
    for k in kernels:
        name = names.get(k["name"])
        if name is None:
            continue
        missing = [f for f in FIELDS if f not in k]
        assert not missing, f"{name}: no {missing} in the metadata"
        out[name] = {f: int(k[f]) for f in FIELDS}
    return out


def kernel_names(exe: str) -> dict:
    """{mangled: name as the launch records spell it} of every kernel the
    harness's object registers."""
    out = subprocess.run([exe, "--kernels"], capture_output=True, text=True, check=True).stdout
    return dict(line.split("\t") for line in out.splitlines())


def golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    table = {k: v for k, v in read(kernel_names(os.path.join(REPO, "build", "c", "launch_check"))).items()
             if k.startswith("md5hip::")}
    doc = {"compiler": compiler_version(),
           "kernels": {k: {"vgpr_count": v["vgpr_count"], "sgpr_spill_count": v["sgpr_spill_count"]}
                       for k, v in sorted(table.items())}}
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    else:
        json.dump({"compiler": doc["compiler"], "kernels": table}, sys.stdout, indent=1)
        print()
