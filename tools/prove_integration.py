#!/usr/bin/env python3
"""Compile proof of INTEGRATION.md §2 against the reference's REAL factory (src/core/IVQVAECodec.{hpp,cpp}).

Compiling needs the reference checkout (read-only; $VQVDB_REFERENCE, or found beside the repository: find_reference()).
Nothing of it is copied into this repository: the two files are copied to a temporary directory, patched there exactly as
INTEGRATION.md §2 says, compiled with -DENABLE_HIP_BACKEND together with the adapter include/vqvdb_hip_backend.hpp, linked against
vqvdb_amd/libvqvdb_hip.so, and the temporary directory is deleted.  Only the executables are kept.

Checks:
  1. the patched reference factory + HipBackend compile and link (g++ -std=c++17 -Wall -Wextra, no warnings from our header);
  2. IVQVAECodec::create(cfg{CUDA, "/nonexistent/model.vqw"}, BackendType::HIP) returns nullptr and prints the reference's
     "Failed to create VQ-VAE backend: ..." line on stderr (IVQVAECodec.cpp:106-109) — no GPU needed: the pack is opened first;
  3. BackendType::LibTorch / ::ONNX keep their numeric values (0, 1) and HIP is 2;
  4. create(cfg, BackendType::ONNX) in this build (ONNX disabled) still takes the reference's default branch -> nullptr.

  5. INTEGRATION.md §3 (the SOP diff): the one-line change `BackendType::ONNX` -> `BackendType::HIP` is applied to temporary copies of
     the reference's real src/SOP/SOP_VQVDB_Encoder.cpp and SOP_VQVDB_Decoder.cpp (anchors asserted), the statements of their
     initializeCodec() from `CodecConfig config;` to the `create(...)` call are lifted VERBATIM out of the patched text into a test
     function (the SOP files themselves need the Houdini SDK and cannot be compiled here), and compiled against the patched real
     factory with a weight pack embedded in each documented way: this repository's generator
     (`python -m vqvdb_amd.weightpack --header`, header mode and object mode) and the reference's own python/convert_to_header.py
     with `--name g_vqhip_pack_data`.  On this GPU-less box `create({CUDA, EmbeddedModel{}}, HIP)` must fail at the DEVICE
     ("no HIP device available"), i.e. after the embedded pack was found and parsed — never with "no weight pack given";
     a build without an embedded pack must fail with exactly that message.

    python tools/prove_integration.py                 -> compile into a temporary directory and run: exit code 0 and "integration proof: OK"
    python tools/prove_integration.py --build DIR     -> compile only (__graft_entry__.build() -> oracle/ref_build.py: DIR = oracle/_ref/integration)
    python tools/prove_integration.py --run DIR [--gpu]  -> run what --build compiled (no reference needed); --gpu: a device is present
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def find_reference() -> str:
    """The reference checkout: $VQVDB_REFERENCE, else a directory `reference` beside this repository or beside one of its parent
    directories, else ~/reference.  The first candidate when none holds src/core (the caller then skips)."""
    if os.environ.get("VQVDB_REFERENCE"):
        return os.environ["VQVDB_REFERENCE"]
    cands, d = [], ROOT
    while os.path.dirname(d) != d:
        d = os.path.dirname(d)
        cands.append(os.path.join(d, "reference"))
    cands.append(os.path.join(os.path.expanduser("~"), "reference"))
    return next((c for c in cands if os.path.isdir(os.path.join(c, "src", "core"))), cands[0])


REF_ROOT = find_reference()
REF = os.path.join(REF_ROOT, "src", "core")
LIB = os.path.join(ROOT, "vqvdb_amd", "libvqvdb_hip.so")

MAIN = r'''
#include <cstdio>
#include "core/IVQVAECodec.hpp"
static_assert(static_cast<int>(BackendType::LibTorch) == 0 && static_cast<int>(BackendType::ONNX) == 1 && static_cast<int>(BackendType::HIP) == 2,
              "appending HIP must not renumber the existing backends");
int main() {
	CodecConfig cfg;
	cfg.device = CodecConfig::Device::CUDA;
	cfg.source = std::filesystem::path("/nonexistent/model.vqw");
	std::unique_ptr<IVQVAECodec> a = IVQVAECodec::create(cfg, BackendType::HIP);
	std::unique_ptr<IVQVAECodec> b = IVQVAECodec::create(cfg, BackendType::ONNX);
	cfg.device = CodecConfig::Device::CPU;
	std::unique_ptr<IVQVAECodec> c = IVQVAECodec::create(cfg, BackendType::HIP);
	std::printf("hip_missing_pack=%s onnx_disabled=%s hip_cpu_device=%s\n", a ? "object" : "nullptr", b ? "object" : "nullptr", c ? "object" : "nullptr");
	return (a || b || c) ? 1 : 0;
}
'''


def patch_sources(src_dir: str) -> None:
    hpp = os.path.join(src_dir, "core", "IVQVAECodec.hpp")
    cpp = os.path.join(src_dir, "core", "IVQVAECodec.cpp")
    h = open(hpp).read()
    old = "enum class BackendType { LibTorch, ONNX };"
    assert h.count(old) == 1, "INTEGRATION.md §2 anchor (BackendType enum) not found in the reference header"
    open(hpp, "w").write(h.replace(old, "enum class BackendType { LibTorch, ONNX, HIP };"))
    c = open(cpp).read()
    inc_anchor = "#ifdef ENABLE_TORCH_BACKEND\n#include \"backends/torch/TorchBackend.hpp\"\n#endif\n"
    assert c.count(inc_anchor) == 1, "INTEGRATION.md §2 anchor (backend includes) not found in the reference factory"
    c = c.replace(inc_anchor, inc_anchor + "\n#ifdef ENABLE_HIP_BACKEND\n#include \"backends/hip/HipBackend.hpp\"\n#endif\n")
    case_anchor = "\t\t\tdefault:\n\t\t\t\tthrow std::runtime_error(\n\t\t\t\t    \"Requested backend type is not available"
    assert c.count(case_anchor) == 1, "INTEGRATION.md §2 anchor (factory switch default) not found in the reference factory"
    c = c.replace(case_anchor, "#ifdef ENABLE_HIP_BACKEND\n\t\t\tcase BackendType::HIP:\n\t\t\t\treturn std::unique_ptr<IVQVAECodec>(new HipBackend(config));\n#endif\n" + case_anchor)
    open(cpp, "w").write(c)


SOP_FILES = ("SOP_VQVDB_Encoder.cpp", "SOP_VQVDB_Decoder.cpp")
SOP_OLD = "IVQVAECodec::create(config, BackendType::ONNX);"
SOP_NEW = "IVQVAECodec::create(config, BackendType::HIP);"


def sop_init_statements() -> list:
    """INTEGRATION.md §3 applied to the text of the two SOPs; returns, per SOP, the statements from `CodecConfig config;`
    through the patched create() call — what the SOP will execute to get its backend."""
    out = []
    for f in SOP_FILES:
        t = open(os.path.join(REF_ROOT, "src", "SOP", f)).read()
        assert t.count(SOP_OLD) == 1, f"INTEGRATION.md §3 anchor not found exactly once in {f}"
        t = t.replace(SOP_OLD, SOP_NEW)
        a = t.index("CodecConfig config;")
        b = t.index(SOP_NEW) + len(SOP_NEW)
        block = t[a:b]
        assert "config.source = EmbeddedModel{};" in block and "config.device = CodecConfig::Device::CUDA;" in block, f"{f}: SOP no longer hard-codes CUDA + EmbeddedModel"
        out.append((f, block))
    return out


SOP_MAIN = r'''
#include <cstdio>
#include <memory>
#include "core/IVQVAECodec.hpp"
%s
int main() {
	const bool a = sop_0(), b = sop_1();
	std::printf("sop_encoder_backend=%%s sop_decoder_backend=%%s\n", a ? "object" : "nullptr", b ? "object" : "nullptr");
	return 0;
}
'''


# the SOP route executables: file name, what was compiled in, whether a pack is embedded
SOP_BUILDS = [("sop_own_header", "weightpack --header, included by the adapter", True),
              ("sop_own_object", "weightpack --header, linked as its own object", True),
              ("sop_ref_tool", "reference convert_to_header.py --name g_vqhip_pack_data", True),
              ("sop_no_pack", "no embedded pack in the build", False)]


def tiny_pack() -> bytes:
    """Parses; the device check comes before the shape validation (the same pack as tests/test_host_logic.py's _tiny_pack)."""
    sys.path.insert(0, ROOT)
    import numpy as np
    from vqvdb_amd import weightpack
    return weightpack.dumps({"encoder.pre.0.bias": np.arange(16, dtype=np.float32)})


def build_sop_embedded(tmp: str, src: str, out: str) -> bool:
    fns = "".join("static bool sop_%d() {\n\t// %s, INTEGRATION.md §3 applied\n\t%s\n\treturn backend != nullptr;\n}\n" % (i, f, block)
                  for i, (f, block) in enumerate(sop_init_statements()))
    open(os.path.join(tmp, "sop_main.cpp"), "w").write(SOP_MAIN % fns)
    vqw = os.path.join(tmp, "model.vqw")
    open(vqw, "wb").write(tiny_pack())
    own = os.path.join(tmp, "own")
    ref = os.path.join(tmp, "ref")
    os.makedirs(os.path.join(own, "bin"))
    os.makedirs(os.path.join(ref, "bin"))
    r = subprocess.run([sys.executable, "-m", "vqvdb_amd.weightpack", "--header", vqw, os.path.join(own, "bin", "vqhip_pack.h")], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([sys.executable, os.path.join(REF_ROOT, "python", "convert_to_header.py"), vqw, os.path.join(ref, "bin", "vqhip_pack.h"), "--name", "g_vqhip_pack_data"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    obj = os.path.join(tmp, "vqhip_pack.o")
    subprocess.run(["gcc", "-x", "c", "-c", os.path.join(own, "bin", "vqhip_pack.h"), "-o", obj], check=True)
    base = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-DENABLE_HIP_BACKEND", "-I", src, "-I", os.path.join(src, "core"),
            os.path.join(src, "core", "IVQVAECodec.cpp"), os.path.join(tmp, "sop_main.cpp")]
    link = ["-L" + os.path.dirname(LIB), "-lvqvdb_hip", "-Wl,-rpath," + os.path.dirname(LIB)]
    extras = {"sop_own_header": ['-DVQVDB_HIP_EMBEDDED_PACK_HEADER="bin/vqhip_pack.h"', "-I", own],
              "sop_own_object": ["-DVQVDB_HIP_EMBEDDED_PACK", obj],
              "sop_ref_tool": ['-DVQVDB_HIP_EMBEDDED_PACK_HEADER="bin/vqhip_pack.h"', "-I", ref],
              "sop_no_pack": []}
    ok = True
    for exe, name, _ in SOP_BUILDS:
        r = subprocess.run(base + extras[exe] + ["-o", os.path.join(out, exe)] + link, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stderr[-3000:])
            print(f"  SOP route [{name}]: FAILED to compile/link")
            ok = False
    # test_embedded_model_builds_link_and_reach_the_device: leaf_harness with a header written by the reference's own generator
    from vqvdb_amd.build import build_harness_embedded
    build_harness_embedded(tiny_pack(), os.path.join(out, "harness_ref_tool"), "header", os.path.join(REF_ROOT, "python", "convert_to_header.py"))
    return ok


def build_proofs(out: str) -> bool:
    """Compile the patched reference factory (+ MAIN) and the SOP route executables into `out`."""
    sys.path.insert(0, ROOT)
    from vqvdb_amd.build import build
    build()
    os.makedirs(out, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="vqhip_integration_")
    try:
        src = os.path.join(tmp, "src")
        os.makedirs(os.path.join(src, "core"))
        os.makedirs(os.path.join(src, "backends", "hip"))
        for f in ("IVQVAECodec.hpp", "IVQVAECodec.cpp"):
            shutil.copyfile(os.path.join(REF, f), os.path.join(src, "core", f))      # contents only: the reference is read-only, the copy is patched
        shutil.copy(os.path.join(ROOT, "include", "vqvdb_hip.h"), os.path.join(src, "backends", "hip", "vqvdb_hip.h"))
        shutil.copy(os.path.join(ROOT, "include", "vqvdb_hip_backend.hpp"), os.path.join(src, "backends", "hip", "HipBackend.hpp"))
        patch_sources(src)
        open(os.path.join(tmp, "main.cpp"), "w").write(MAIN)
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-DENABLE_HIP_BACKEND", "-I", src, "-I", os.path.join(src, "core"),
               os.path.join(src, "core", "IVQVAECodec.cpp"), os.path.join(tmp, "main.cpp"), "-o", os.path.join(out, "proof"),
               "-L" + os.path.dirname(LIB), "-lvqvdb_hip", "-Wl,-rpath," + os.path.dirname(LIB)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stderr)
            print("integration proof: FAILED (compile/link)")
            return False
        ours = [ln for ln in r.stderr.splitlines() if "HipBackend.hpp" in ln or "vqvdb_hip.h" in ln]
        if ours:
            print("\n".join(ours))
            print("integration proof: FAILED (warnings from the adapter headers)")
            return False
        return build_sop_embedded(tmp, src, out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run_proofs(out: str, gpu: bool = False) -> bool:
    """Run what build_proofs compiled.  Without a device, the embedded builds must fail at the DEVICE ("no HIP device available");
    with one (gpu=True), they get past it and the tiny pack is refused by the shape validation — never "no weight pack given"."""
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(LIB) + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([os.path.join(out, "proof")], capture_output=True, text=True, env=env)
    print(r.stdout.strip())
    print("stderr of the patched reference factory:\n  " + "\n  ".join(r.stderr.strip().splitlines()))
    ok = (r.returncode == 0 and "hip_missing_pack=nullptr onnx_disabled=nullptr hip_cpu_device=nullptr" in r.stdout
          and r.stderr.count("Failed to create VQ-VAE backend:") == 3 and "Model file not found at path: /nonexistent/model.vqw" in r.stderr)
    for exe, name, embedded in SOP_BUILDS:
        r = subprocess.run([os.path.join(out, exe)], capture_output=True, text=True, env=env)
        msgs = [ln for ln in r.stderr.splitlines() if ln.startswith("Failed to create VQ-VAE backend:")]
        if embedded:
            good = len(msgs) == 2 and (gpu or all("no HIP device available" in m for m in msgs)) and "no weight pack given" not in r.stderr
        else:
            good = len(msgs) == 2 and all("no weight pack given (embedded model absent from this build)" in m for m in msgs)
        print(f"  SOP route [{name}]: {r.stdout.strip()} | {msgs[0] if msgs else r.stderr.strip()} -> {'ok' if good else 'FAILED'}")
        ok = ok and good
    print("integration proof: " + ("OK" if ok else "FAILED"))
    return ok


def main(argv) -> int:
    if "--run" in argv:
        return 0 if run_proofs(argv[argv.index("--run") + 1], gpu="--gpu" in argv) else 1
    if not os.path.isdir(REF):
        print(f"integration proof: SKIPPED (no reference checkout at {REF_ROOT}; set VQVDB_REFERENCE)")
        return 0
    if "--build" in argv:
        return 0 if build_proofs(argv[argv.index("--build") + 1]) else 1
    tmp = tempfile.mkdtemp(prefix="vqhip_integration_out_")
    try:
        return 0 if build_proofs(tmp) and run_proofs(tmp) else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.exit(main(sys.argv[1:]))
