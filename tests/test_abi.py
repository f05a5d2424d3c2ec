"""CPU-side checks of the C-ABI boundary: the shared library loads and exports every symbol
include/owl_hip.h declares (no compute calls without a GPU)."""
import ctypes
import os

import pytest

from owl_vit_object_detection_amd import _lib


def _TUNING_BUILD():
    """Is the loaded libowlhip.so an OWL_TUNING build?  Asked of the library, not of the environment."""
    from owl_vit_object_detection_amd import _lib as _L
    try:
        return _L.is_tuning_build()
    except _L.OwlLibError:
        return False



@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_parses():
    protos = _lib.parse_header()
    assert "owl_gemm_nt_bf16" in protos and "owl_last_error" in protos
    ret, args = protos["owl_gemm_nt_bf16"]
    assert ret == "int" and args[0] == ("void*", "stream") and len(args) == 21 and args[-1] == ("int", "tile")
    for name, (ret, args) in protos.items():
        for ty, _ in args:
            assert ty in _lib._CTYPES, (name, ty)


def test_library_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.parse_header():
        assert hasattr(lib, name), f"{name} declared in include/owl_hip.h but not exported"
    assert built.owl_abi_version() == _lib.header_abi_version() >= 3


def test_no_process_global_setters_in_the_product_abi(built):
    """re-entrant, no global mutable state.  The tuning switches (kernel-choice override, store skipping,
    attention debug flags) must be neither declared in the product header nor exported by the default build."""
    protos = _lib.parse_header()
    banned = ("owl_gemm_set_tile", "owl_gemm_set_persistent", "owl_gemm_debug_nostore", "owl_gemm_debug_slots", "owl_attention_debug")
    for name in banned:
        assert name not in protos, name
    assert not any("_set_" in n or "_debug" in n for n in protos), [n for n in protos if "_set_" in n or "_debug" in n]
    if not _TUNING_BUILD():
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in banned:
            assert not hasattr(lib, name), f"{name} exported by the default build"
    # every op that needs device scratch has a size query
    for q in ("owl_postprocess_workspace", "owl_box_final_bwd_blocks", "owl_gemm_effective_splits", "owl_gemm_tn_slab_workspace_bytes",
              "owl_attention_bwd_workspace_bytes", "owl_gemm_slab_workspace_bytes", "owl_gemm_nt_plan"):
        assert q in protos, q


def test_argument_validation_sets_error_without_gpu(built):
    # argument checks run before any HIP call: safe without a device
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        _lib.call("owl_gemm_nt_bf16", None, 0, None, 0, 0, None, 0, 0, None, None, 0, None, None, 0, 1, 4, 64, 1.0, 1, 0, 0)
    assert "null pointer" in _lib.last_error()
    # the patch gathers (epilogues 7, 12) run through owl_patch_embed_bf16 only, whatever the shape: refused before any kernel is chosen (the pointers
    # are host memory nothing reads)
    import torch
    h = torch.zeros(8)
    for epi in (7, 12):
        for (M, N, K) in ((128, 128, 64), (4096, 1024, 768)):
            with pytest.raises(_lib.OwlLibError, match=f"unknown epilogue {epi}"):
                _lib.call("owl_gemm_nt_bf16", None, epi, h, K, M, h, K, N, None, h, N, None, None, 0, M, N, K, 1.0, 1, 0, 0)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No CPU / eager fallback: without libowlhip.so every op raises (the product path never routes through the oracle)."""
    from owl_vit_object_detection_amd import _lib as L
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "libowlhip.so"))
    with pytest.raises(L.OwlLibError, match="no CPU fallback|not found"):
        L.load()
    with pytest.raises(L.OwlLibError):
        L.call("owl_abi_version")


def test_abi_version_mismatch_is_refused(built, monkeypatch, tmp_path):
    """A binding generated from a header of another ABI version must not drive the library (changed argument lists / scratch layouts)."""
    from owl_vit_object_detection_amd import _lib as L
    hdr = tmp_path / "owl_hip.h"
    hdr.write_text(open(L.HEADER).read().replace(f"#define OWL_ABI_VERSION {L.header_abi_version()}", "#define OWL_ABI_VERSION 9999"))
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "HEADER", str(hdr))
    with pytest.raises(L.OwlLibError, match="OWL_ABI_VERSION"):
        L.load()


def test_product_package_never_imports_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/: NO file of the product package imports it (round 6: the
    smoke check moved out of the package, so there is no exception to make)."""
    import os
    import re
    pkg = os.path.dirname(os.path.abspath(__import__("owl_vit_object_detection_amd").__file__))
    offenders = []
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) or "owl_oracle" in src:
                offenders.append(fn)
    assert offenders == []


def test_dynamic_symbol_table_holds_only_the_c_abi(built):
    """the library is built with -fvisibility=hidden + a linker version script (csrc/libowlhip.map): its dynamic symbol table DEFINES the
    entry points of include/owl_hip.h and nothing else -- no `__device_stub__` kernel stubs, no kernel handles, no C++ helpers."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    declared = set(_lib.parse_header())
    stray = sorted(n for n in defined if not n.startswith("owl_"))
    assert stray == [], stray[:10]
    if not _TUNING_BUILD():
        assert defined == declared, (sorted(defined - declared), sorted(declared - defined))


# ---- register budget of the hot kernels (no GPU needed: the code objects' metadata) -------------------------------------------------------
_LLVM = "/opt/rocm/lib/llvm/bin"
# kernel (mangled-name pattern) -> VGPRs allowed in scratch.  0 everywhere on the hot path; the one exception says why.
_SPILL_FREE = {
    "gemm_pp2.o": [r"gemm_pp2_kernelILi0ELb0ELb0E", r"gemm_pp2_kernelILi0ELb0ELb1E", r"gemm_pp2_kernelILi1ELb0ELb0E", r"gemm_pp2_kernelILi8ELb0ELb0E", r"gemm_pp2_kernelILi7ELb0ELb0E",
                   r"gemm_pp2_kernelILi2E", r"gemm_pp2_kernelILi9E", r"gemm_pp2_kernelILi4E", r"gemm_pp2_kernelILi10E", r"gemm_pp2_kernelILi12E"],
    "gemm_pph.o": [r"gemm_pph_kernelILi0E"],
    "attention_fwd.o": [r"attn_fwd_kernelILb1ELb1ELi4E", r"attn_fwd_kernelILb1ELb0ELi4E"],
    "attention_bwd.o": [r"attn_bwd_dq_kernel", r"attn_dvec_kernel"],
    "gemm_tn.o": [r"gemm_tn_pp_kernel"],
    "norm.o": [r"ln_fwd_kernel", r"merge_ln_kernel"],
    "backward.o": [r"ln_bwd_kernel"],
}
# attn_bwd_dkdv: two lane-id-derived values (l31, 8 * hi) are parked in scratch BEFORE the query-tile loop and reloaded AFTER it for the output addresses
# (one scratch_store pair in the prologue, one scratch_load pair in the epilogue; nothing inside the loop -- checked on the assembly)
_SPILL_ALLOWED = {"attention_bwd.o": {r"attn_bwd_dkdv_kernel": 2}}


def _kernel_notes(obj):
    """{kernel name: {spill, scratch, vgpr}} from the gfx950 code object bundled in a host object (its AMDGPU metadata note is YAML)."""
    import subprocess
    import tempfile
    import yaml
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "k.co")
        subprocess.run([f"{_LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj], check=True)
        subprocess.run([f"{_LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}", "--unbundle"], check=True)
        notes = subprocess.run([f"{_LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    doc = notes[notes.index("---"):]
    doc = doc[:doc.index("\n...")] if "\n..." in doc else doc
    meta = yaml.safe_load(doc)
    return {k[".name"]: dict(spill=int(k[".vgpr_spill_count"]), scratch=int(k[".private_segment_fixed_size"]), vgpr=int(k[".vgpr_count"])) for k in meta["amdhsa.kernels"]}


def test_hot_kernels_do_not_spill(built):
    """VERDICT r04 #2 rider: `vgpr_spill_count == 0` for the GEMM / attention / LayerNorm kernels of the train step, read from the metadata of the very
    objects libowlhip.so is linked from (round 4 shipped gemm_pp2<8> with 8 and <7> with 14 spilled VGPRs, attn_fwd with 5)."""
    import re
    bdir = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "build")
    if not os.path.exists(os.path.join(bdir, "gemm_pp2.o")):
        import __graft_entry__ as g
        g.build()
    for obj, pats in _SPILL_FREE.items():
        ks = _kernel_notes(os.path.join(bdir, obj))
        assert ks, obj
        for pat in pats:
            hits = {k: v for k, v in ks.items() if re.search(pat, k)}
            assert hits, (obj, pat, sorted(ks))
            for k, v in hits.items():
                assert v["spill"] == 0 and v["scratch"] == 0, (k, v)
    for obj, allowed in _SPILL_ALLOWED.items():
        ks = _kernel_notes(os.path.join(bdir, obj))
        for pat, cap in allowed.items():
            hits = {k: v for k, v in ks.items() if re.search(pat, k)}
            assert hits, (obj, pat)
            for k, v in hits.items():
                assert v["spill"] <= cap, (k, v)


def test_patch_embed_scratch_query_is_the_dispatchers_rule(built):
    """the Python side sizes the im2row scratch of owl_patch_embed_bf16 from the library's own query (host function, no GPU): 0 where the chosen
    kernel gathers from the image itself -- every 2^n patch size, any patch size on the ping-pong kernel --, the im2row matrix otherwise; odd patch sizes refused."""
    import torch

    def q(B, S, ps, D, tile=0):
        n = torch.zeros(1, dtype=torch.int64)
        _lib.call("owl_patch_embed_scratch_bytes", B, S, ps, D, tile, n)
        return int(n.item())

    assert q(32, 768, 16, 768) == 0 and q(1, 768, 16, 768) == 0 and q(1, 96, 16, 64) == 0          # 2^n patch sizes: never
    assert q(16, 840, 14, 1024) == 0 and q(1, 840, 14, 1024) == 0                                   # L/14: the ping-pong kernel at every batch size
    small = q(3, 84, 14, 128)                                                                       # tiny-l14: a problem too small for the ping-pong kernel
    rows = (3 * 36 + 127) // 128 * 128
    assert small == rows * 704 * 2                                                                  # [rows128(B*P), Kg = 3*14*16 -> 704] bf16
    assert q(3, 84, 14, 128, tile=7) == 0 and q(16, 840, 14, 1024, tile=256) > 0                    # a pinned kernel follows the same rule
    with pytest.raises(_lib.OwlLibError):
        q(1, 90, 15, 128)
