"""CPU-only checks of the host side: weight pack round trip, the C-ABI library loads and
exports every symbol include/vqvdb_hip.h declares, header/ctypes agreement, and the
no-GPU failure mode (loud error, no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from vqvdb_amd import codec as vc
from vqvdb_amd import synth, weightpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weightpack_roundtrip(weights, tmp_path):
    blob = weightpack.dumps(weights)
    back = weightpack.loads(blob)
    assert list(back) == [t[0] for t in synth.TENSORS]
    for k, v in weights.items():
        assert back[k].shape == v.shape and np.array_equal(back[k], v)
    p = tmp_path / "model.vqw"
    weightpack.save(p, weights)
    assert np.array_equal(weightpack.load(p)["encoder.down.weight"], weights["encoder.down.weight"])
    with pytest.raises(ValueError):
        weightpack.loads(b"garbage-garbage-")


def test_from_state_dict_drops_training_buffers(weights):
    sd = dict(weights)
    sd["quantizer.cluster_size"] = np.ones(256, np.float32)
    sd["quantizer.embed_avg"] = weights["quantizer.embedding"].copy()
    out = weightpack.from_state_dict(sd)
    assert set(out) == set(weights)


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "vqvdb_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vqhip_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from vqvdb_amd.build import build
    lib = ctypes.CDLL(build())
    declared = _declared_symbols()
    assert sorted(vc.ABI_SYMBOLS) == declared
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in ctypes.cast(lib.vqhip_version, ctypes.CFUNCTYPE(ctypes.c_char_p))()


def test_create_fails_loudly_without_gpu_or_pack(weights, capsys):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the failure path is covered by the -m gpu tests")
    with pytest.raises(RuntimeError, match="no HIP device|hip"):
        vc.HipCodec(weightpack.dumps(weights))
    be = vc.IVQVAECodec.create(vc.CodecConfig(device=vc.CodecConfig.Device.CUDA, source=weightpack.dumps(weights)), vc.BackendType.HIP)
    assert be is None and "Failed to create VQ-VAE backend" in capsys.readouterr().err
    with pytest.raises(RuntimeError, match="bad magic"):
        vc.HipCodec(b"x" * 64)


def test_vqvdb_stream_framing_roundtrip(tmp_path):
    """The OpenVDB-free .vqvdb v3 reader/writer (vqvdb_amd/host/vqvdb_stream.hpp) against the byte
    layout of SURVEY.md App. B, parsed independently here."""
    import struct
    import subprocess
    from vqvdb_amd.build import build, build_harness
    build()
    exe = build_harness()
    path = tmp_path / "t.vqvdb"
    assert subprocess.run([exe, "streamtest", str(path)], capture_output=True).returncode == 0
    raw = path.read_bytes()
    magic, ver, ngrids, nemb, ndim = struct.unpack_from("<5sBBIB", raw, 0)
    assert (magic, ver, ngrids, nemb, ndim) == (b"VQVDB", 3, 2, 256, 3)
    off, total = 12, 0
    for expect_name, expect_blocks in ((b"density", 700), (b"temperature", 300)):
        (nl,) = struct.unpack_from("<I", raw, off); off += 4
        assert raw[off:off + nl] == expect_name; off += nl
        off += 64
        assert struct.unpack_from("<3H", raw, off) == (4, 4, 4); off += 6
        (nb,) = struct.unpack_from("<I", raw, off); off += 4
        assert nb == expect_blocks
        x, y, z = struct.unpack_from("<3i", raw, off)           # first chunk: origin then 64 index bytes
        assert (x, y, z) == (8 * (total % 1024), 8 * ((total // 1024) % 1024), 0)
        off += nb * 76; total += nb
    assert off == len(raw) and total == 1000


def test_vqvdbfile_numpy_matches_cpp_writer(tmp_path):
    """vqvdb_amd/vqvdbfile.py (numpy framing used by the stream parity tests) parses the file the C++ writer
    produced and re-serialises it to the same bytes; truncated / foreign files are rejected with the reader's messages."""
    import subprocess
    from vqvdb_amd import vqvdbfile
    from vqvdb_amd.build import build, build_harness
    build()
    exe = build_harness()
    path = tmp_path / "t.vqvdb"
    assert subprocess.run([exe, "streamtest", str(path)], capture_output=True).returncode == 0
    raw = path.read_bytes()
    grids = vqvdbfile.loads(raw)
    assert [g.name for g in grids] == ["density", "temperature"] and [len(g.origins) for g in grids] == [700, 300]
    assert grids[1].transform[0] == 1.5 and grids[0].indices.dtype == np.uint8
    assert vqvdbfile.dumps(grids) == raw
    with pytest.raises(ValueError, match="truncated"):
        vqvdbfile.loads(raw[:-10])
    with pytest.raises(ValueError, match="magic"):
        vqvdbfile.loads(b"OPENVDB" + raw[7:])
    empty = [vqvdbfile.Grid("e", np.zeros((0, 3), np.int32), np.zeros((0, 64), np.uint8))]
    assert len(vqvdbfile.loads(vqvdbfile.dumps(empty))[0].origins) == 0


def test_full_training_host_helpers(weights):
    """Flat parameter vector <-> state_dict (the reference's parameter order) and the closed-form cosine schedule."""
    import math
    import torch
    from vqvdb_amd import full_training as ft
    flat = ft.dict_to_flat(weights)
    assert flat.size == 995905 and flat.dtype == np.float32
    back = ft.flat_to_dict(flat)
    assert list(back) == [n for n, _ in ft.TRAINABLE] and all(np.array_equal(back[k], weights[k]) for k in back)
    assert "quantizer.embedding" not in back
    with pytest.raises(ValueError):
        ft.flat_to_dict(flat[:-1])
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-4)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=50)
    for step in range(50):
        assert math.isclose(ft.cosine_lr(1e-4, step, 50), sch.get_last_lr()[0], rel_tol=1e-9, abs_tol=1e-15)
        opt.step()
        sch.step()


def _patch_entry(pack: bytes, name: str, **fields) -> bytes:
    """Rewrite fields (off / count / dims) of one table entry of a VQWPACK1 blob."""
    buf = bytearray(pack)
    n = weightpack._HEAD.unpack_from(buf, 0)[1]
    for i in range(n):
        pos = weightpack._HEAD.size + i * weightpack._ENTRY.size
        rec = list(weightpack._ENTRY.unpack_from(buf, pos))
        if rec[0].rstrip(b"\0").decode() == name:
            if "off" in fields:
                rec[8] = fields["off"]
            if "count" in fields:
                rec[9] = fields["count"]
            buf[pos:pos + weightpack._ENTRY.size] = weightpack._ENTRY.pack(*rec)
            return bytes(buf)
    raise KeyError(name)


def test_malformed_weight_pack_bounds_are_checked_before_any_read(weights):
    """a user-supplied pack must not make vqhip_create read out of bounds — count/offset overflow, and a table entry
    whose count disagrees with its dims (consumers read prod(dims) floats).  parse_pack runs before any device is touched."""
    pack = weightpack.dumps(weights)
    cases = {
        "count overflows u64 when multiplied by 4": dict(count=(1 << 62) + 5),
        "offset beyond the file": dict(off=(1 << 63)),
        "offset + count wraps": dict(off=len(pack) - 4, count=(1 << 62)),
    }
    for what, f in cases.items():
        with pytest.raises(RuntimeError, match="out of bounds"):
            vc.HipCodec(_patch_entry(pack, "decoder.up_conv.weight", **f))
    with pytest.raises(RuntimeError, match="count does not match its shape"):     # right dims, short count
        vc.HipCodec(_patch_entry(pack, "decoder.up_conv.weight", count=16))
    with pytest.raises(RuntimeError, match="count does not match its shape"):
        vc.HipCodec(_patch_entry(pack, "encoder.pre.0.bias", count=17))


def test_python_wrappers_validate_leaf_buffers():
    ok = [np.zeros(512, np.float32) for _ in range(3)]
    assert len(vc.HipCodec._leaf_ptrs(ok, 3, writable=True)) == 3
    for bad in ([np.zeros(512, np.float64)] * 3, [np.zeros(511, np.float32)] * 3, [np.zeros((512, 2), np.float32)[:, 0]] * 3, ok[:2]):
        with pytest.raises(ValueError):
            vc.HipCodec._leaf_ptrs(bad, 3, writable=False)
    ro = np.zeros(512, np.float32)
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        vc.HipCodec._leaf_ptrs([ro], 1, writable=True)


def test_rank_cpu_plan_is_a_partition():
    from vqvdb_amd.sharding import _parse_cpulist, plan_rank_cpus
    assert _parse_cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11]
    allowed = list(range(96))
    sets = [plan_rank_cpus(allowed, r, 8) for r in range(8)]
    assert all(len(s) == 12 for s in sets) and sorted(sum(sets, [])) == allowed
    # two NUMA nodes, four GPUs each: ranks sharing a node split that node's cores
    node1 = list(range(48, 96))
    s = [plan_rank_cpus(allowed, 4 + k, 8, node1, 4, k) for k in range(4)]
    assert sorted(sum(s, [])) == node1
    # fewer CPUs than ranks (a 2-CPU container): no binding rather than an empty set
    assert plan_rank_cpus([0, 1], 5, 8) == [0, 1]
    # NUMA node outside the allowed mask: falls back to the even split
    assert plan_rank_cpus(list(range(16)), 1, 2, list(range(64, 128)), 1, 0) == list(range(8, 16))
    # an inconsistent slot (numa_slot >= numa_peers) never yields an empty set: even split
    assert plan_rank_cpus(allowed, 5, 8, node1, 4, 4) == list(range(60, 72))
    # interleaved GPU -> node mapping (even ranks on node 0, odd on node 1): with the gathered node list every rank gets its own slice
    nodes = [r % 2 for r in range(8)]
    node_cpus = {0: list(range(0, 48)), 1: node1}
    sets = []
    for r in range(8):
        same = [q for q, nd in enumerate(nodes) if nd == nodes[r]]
        sets.append(plan_rank_cpus(allowed, r, 8, node_cpus[nodes[r]], len(same), same.index(r)))
    assert all(len(x) == 12 for x in sets) and sorted(sum(sets, [])) == allowed


def test_hostbench_index_file_writer_matches_numpy_framing(tmp_path):
    """The chunked single-grid writer used for the multi-million-leaf configs[2] files produces the App. B bytes."""
    from vqvdb_amd import hostbench, vqvdbfile
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 256, size=(1000, 64), dtype=np.uint8)
    p = tmp_path / "w.vqvdb"
    hostbench.write_index_file(str(p), lambda s, k: idx[s:s + k], 1000, chunk=333)
    want = vqvdbfile.dumps([vqvdbfile.Grid("density", hostbench.origins_of(1000), idx)])
    assert p.read_bytes() == want
    g = vqvdbfile.loads(p.read_bytes())[0]
    assert len(np.unique(g.origins, axis=0)) == 1000


def test_integration_diff_compiles_against_the_reference_factory():
    """INTEGRATION.md §2 applied to a temporary copy of the reference's real factory, compiled with the adapter and linked
    against libvqvdb_hip.so (tools/prove_integration.py).  build() compiles it into oracle/_ref/integration from a reference
    checkout (oracle/ref_build.py); this test runs those executables and reads nothing outside the repository."""
    import subprocess
    import sys
    import torch
    out = os.path.join(ROOT, "oracle", "_ref", "integration")
    if not os.path.exists(os.path.join(out, "proof")):
        pytest.skip("oracle/_ref/integration not built (build() found no reference checkout)")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "prove_integration.py"), "--run", out] + (["--gpu"] if torch.cuda.is_available() else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "integration proof: OK" in r.stdout, r.stdout + r.stderr


def _ref_fixture_content():
    import importlib.util
    spec = importlib.util.spec_from_file_location("prove_vqvdb_format", os.path.join(ROOT, "tools", "prove_vqvdb_format.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.fixture_content()


def test_reference_written_vqvdb_fixture_round_trips():
    """tests/golden/ref_writer_v3.vqvdb was written by the reference's REAL VDBStreamWriter (src/Utils/VQVDB_Reader.cpp:58-150),
    compiled in the build container against a size-only stand-in for openvdb/Types.h (tools/prove_vqvdb_format.py, which also runs
    the reference READER over files of both of this repository's writers).  Here: vqvdbfile parses every field of it and
    re-serialises it byte for byte; the C++ StreamReader of vqvdb_stream.hpp (leaf_harness readcheck) sees the same content."""
    from vqvdb_amd import vqvdbfile
    path = os.path.join(ROOT, "tests", "golden", "ref_writer_v3.vqvdb")
    data = open(path, "rb").read()
    grids = vqvdbfile.loads(data)
    assert vqvdbfile.dumps(grids) == data
    want = _ref_fixture_content()
    assert [g.name for g in grids] == ["density", "temperature"]
    for g, (name, org, idx, tr) in zip(grids, want):
        assert g.name == name and tuple(g.latent_shape) == (4, 4, 4)
        assert np.array_equal(g.origins, org) and np.array_equal(g.indices, idx) and np.array_equal(g.transform, tr)
    assert not np.array_equal(grids[1].transform, np.eye(4, dtype=np.float32).reshape(16))      # non-identity transform survives
    harness = os.path.join(ROOT, "vqvdb_amd", "host", "leaf_harness")
    if os.path.exists(harness):      # built by __graft_entry__.build(); the C++ reader over the reference writer's bytes
        import subprocess
        for batch in ("97", "4096"):
            r = subprocess.run([harness, "readcheck", path, batch], capture_output=True, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            assert "2 grids, 1000 leaves" in r.stdout


def _tiny_pack():
    """A structurally valid VQWPACK1 pack (one tensor): passes the parser, so vqhip_create reaches the device check."""
    return weightpack.dumps({"encoder.pre.0.bias": np.arange(16, dtype=np.float32)})


def test_header_embedder_output(weights, tmp_path):
    """SURVEY §8 f-3's C-header embedder (role of python/convert_to_header.py:4-44): `python -m vqvdb_amd.weightpack --header`
    writes both objects the adapter reads, byte for byte the pack, 12 bytes per line, and refuses non-packs."""
    import subprocess
    import sys
    pk = weightpack.dumps(weights)
    (tmp_path / "m.vqw").write_bytes(pk)
    r = subprocess.run([sys.executable, "-m", "vqvdb_amd.weightpack", "--header", str(tmp_path / "m.vqw"), str(tmp_path / "p.h")],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    text = (tmp_path / "p.h").read_text()
    assert f"g_vqhip_pack_size = {len(pk)};" in text and f"g_vqhip_pack_data[{len(pk)}] = {{" in text
    body = text[text.index("= {\n") + 4:text.index("\n};")]
    rows = body.split("\n")
    assert all(len(row.split(",")) - 1 == 12 for row in rows[:-1])
    got = bytes(int(tok, 16) for tok in re.findall(r"0x[0-9a-f]{2}", body))
    assert got == pk
    with pytest.raises(ValueError):
        weightpack.to_header(b"x" * 256)


def test_embedded_model_builds_link_and_reach_the_device(tmp_path):
    """CodecConfig::source = EmbeddedModel{} — what both reference SOPs hard-code (SOP_VQVDB_Encoder.cpp:63-67,
    SOP_VQVDB_Decoder.cpp:58-62).  Every documented way of compiling a pack in must LINK, and
    IVQVAECodec::create({CUDA, EmbeddedModel{}}, HIP) must get as far as the device: on a box without a GPU it fails with the
    device error, never with "no weight pack given"; a build without a pack refuses EmbeddedModel with exactly that message."""
    import subprocess
    import torch
    from vqvdb_amd import build as vb
    vb.build()
    has_gpu = torch.cuda.is_available()
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))

    def run(exe):
        return subprocess.run([exe, "errors", "@embedded"], capture_output=True, text=True, env=env, timeout=300)

    plain = run(vb.build_harness())
    assert plain.returncode == 1 and "no weight pack given (embedded model absent from this build)" in plain.stderr
    variants = [("default", vb.build_default_embedded_harness())]                       # full synthetic pack, object mode
    variants.append(("header", vb.build_harness_embedded(_tiny_pack(), str(tmp_path / "h_header"), "header")))
    variants.append(("object", vb.build_harness_embedded(_tiny_pack(), str(tmp_path / "h_object"), "object")))
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "vqvdb_amd") + ":" + env["LD_LIBRARY_PATH"]
    ref_tool = os.path.join(ROOT, "oracle", "_ref", "integration", "harness_ref_tool")
    if os.path.exists(ref_tool):      # built by build() from a reference checkout: the header comes from the reference's own generator
        variants.append(("reference tool", ref_tool))
    for name, exe in variants:
        r = run(exe)
        assert "no weight pack given" not in r.stderr, (name, r.stderr)
        if not has_gpu:
            assert r.returncode == 1 and "Failed to create VQ-VAE backend: no HIP device available" in r.stderr, (name, r.stderr)
        elif name == "default":
            assert r.returncode == 0, (name, r.stdout + r.stderr)
        else:                         # the tiny pack parses but is not a VQVAE(1,128,256): refused by the shape validation
            assert r.returncode == 1 and "Failed to create VQ-VAE backend" in r.stderr, (name, r.stderr)
