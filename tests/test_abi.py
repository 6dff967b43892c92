"""The C-ABI library builds for gfx950, loads, and exports every symbol that
include/omg.h declares (no compute calls: this runs without a GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "omg.h")
LIB = os.path.join(ROOT, "octree-mg_amd", "libomg.so")


def declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"\b(omg_[a-z_0-9]+)\s*\(", src)))


def test_header_declares_entry_points():
    names = declared()
    for must in ("omg_ctx_create", "omg_tree_setup", "omg_fas_vcycle", "omg_fas_fmg",
                 "omg_smooth_boxes", "omg_fill_ghost_cells_lvl", "omg_restrict_lvl",
                 "omg_prolong", "omg_update_coarse", "omg_correct_children"):
        assert must in names


def test_library_exports_all_declared_symbols():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "octree-mg_amd", "csrc")], check=True)
    lib = ctypes.CDLL(LIB)
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_python_binding_covers_header():
    from tests.mgdriver import omg
    assert set(declared()) == set(omg.device.SIGNATURES)


def test_library_is_gfx950_code_object():
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-n", LIB],
                         capture_output=True, text=True)
    # the embedded offload bundle names the target
    data = open(LIB, "rb").read()
    assert b"gfx950" in data


def test_library_exports_only_its_own_names():
    """Every defined, non-weak dynamic symbol is an entry point of
    include/omg.h, a name under namespace omg, or the HIP runtime's
    registration data.  User programs link against this library (the Fortran
    drop-in), so a plain global such as a helper left inside the extern "C"
    block would collide with theirs.  (llvm-readelf's GLOBAL binding of a
    defined FUNC / OBJECT / TLS symbol is what nm prints as T, D or B; the
    WEAK ones, nm's W / V, are template instantiations.)"""
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--dyn-syms", "-W", LIB],
                         capture_output=True, text=True, check=True).stdout
    entry_points = set(declared())
    seen, foreign = 0, []
    for line in out.splitlines():
        f = line.split()
        # Num: Value Size Type Bind Vis Ndx Name
        if len(f) != 8 or not f[0].rstrip(":").isdigit() or f[6] == "UND":
            continue
        if f[4] != "GLOBAL" or f[3] not in ("FUNC", "OBJECT", "TLS"):
            continue
        seen += 1
        name = f[7].split("@")[0]
        if not (name in entry_points or name.startswith(("_ZN3omg", "_ZNK3omg", "__hip_"))):
            foreign.append(name)
    assert seen >= len(entry_points)   # (the listing was understood)
    assert not foreign, foreign


def test_last_error_without_gpu_is_clean():
    from tests.mgdriver import omg
    L = omg.device.lib()
    assert isinstance(L.omg_last_error(), bytes)
