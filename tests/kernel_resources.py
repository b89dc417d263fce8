"""What the gfx950 code objects say of each kernel: the AMDGPU metadata notes
(llvm-readelf --notes) of the device ELFs inside build/obj/md5_kernels.o and
build/obj/md5_pages.o, by kernel name as the launch records spell it
("md5hip::md5_desc_fed<true>"; md5_pages.o's kernels, of an unnamed namespace,
without a prefix: "md5_pages_xdma").  md5_pages.o's code object also carries
unreachable copies of md5_kernels.h's kernels under internal names; no launch
names them, and they are not listed.  Metadata only: nothing is disassembled.
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
OBJECTS = (OBJECT, os.path.join(REPO, "build", "obj", "md5_pages.o"))
# md5_pages.hip's kernels, as the launch records spell them (tests/launch_cases.py)
PAGED = ("md5_pages_xdma", "pages_xdma16<md5hip::Crc32PermHasher>", "pages_xdma16<md5hip::Md5Crc32Hasher>",
         "crc32_pages_fast", "md5_update_ctx_pages")
GOLDEN = os.path.join(REPO, "tests", "golden", "kernel_resources.json")
FIELDS = ("agpr_count", "vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
          "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size")


def compiler_version() -> str:
    """hipcc's HIP version and its clang's version line"""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    out = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True)
    return "; ".join(line.strip() for line in out.stdout.splitlines()[:2])


def ours(name: str) -> bool:
    """The product's kernels among those an object registers (rocPRIM's are not)."""
    return name.startswith("md5hip::") or name in PAGED


def read(names: dict, paths=OBJECTS) -> dict:
    """{kernel: {field: int}} for the kernels of the code objects in `paths`
    that `names` ({mangled: name}, from `launch_check --kernels`) lists."""
    out = {}
    for path in paths:
        part = read_object(names, path)
        assert not set(part) & set(out), sorted(set(part) & set(out))
        out.update(part)
    return out


def read_object(names: dict, path: str) -> dict:
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
             if ours(k)}
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
