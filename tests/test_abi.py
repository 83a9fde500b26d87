"""The C ABI without a GPU: libgpi_hip.so loads, exports every entry point that
include/gpi.h declares, the ctypes mirror agrees with the header (declared names,
struct sizes), and the host-only queries answer.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'gpi.h')


def declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r'^\s*(?:int|int64_t|const char\s*\*)\s+(gpi_\w+)\s*\(', src, re.M)))


@pytest.fixture(scope='module')
def lib():
    from gpi import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail('libgpi_hip.so is not built (run __graft_entry__.build())')
    return L


def test_header_declares_the_entry_points():
    names = declared()
    for n in ('gpi_conv_forward', 'gpi_conv_backward', 'gpi_codec_forward', 'gpi_codec_backward', 'gpi_rom',
              'gpi_cgr_residual', 'gpi_adam', 'gpi_head_forward', 'gpi_head_backward', 'gpi_head_form',
              'gpi_wgrad_reduce'):
        assert n in names


def test_library_exports_every_declared_symbol(lib):
    so = C.CDLL(lib.LIB_PATH)
    missing = [n for n in declared() if not hasattr(so, n)]
    assert not missing, missing


def test_ctypes_binding_matches_header(lib):
    assert sorted(lib.SIGNATURES) == declared()


def test_struct_sizes_and_version(lib):
    L = lib.lib()                      # checks every struct size against the ctypes mirror
    assert L.gpi_version() >= 1
    assert L.gpi_error_string(0).decode()
    assert L.gpi_error_string(-2).decode() != L.gpi_error_string(0).decode()


def test_conv_blocks_host_query(lib):
    L = lib.lib()
    d = lib.ConvDesc()
    d.cin, d.cout, d.k, d.stride, d.pad, d.upsample = 10, 5, 3, 1, 1, 0
    d.h_in = d.w_in = d.h_out = d.w_out = 32
    g = lib.Groups()
    g.n_groups = 1
    g.start[0], g.start[1] = 0, 288
    nb = C.c_int32()
    assert L.gpi_conv_blocks(C.byref(d), C.byref(g), C.byref(nb)) == 0
    # full-width tiles of 8 rows on a 32 x 32 plane, one slab row per wave; the 1152 tiles are no multiple of
    # the 256 CUs, so the samples past the first 1024 tiles (256..287) take half-height tiles (GPI_HALF_TILES)
    assert nb.value == (256 * 4 + 32 * 8) * 4
    g.start[1] = 256                    # 1024 tiles: no half tiles
    assert L.gpi_conv_blocks(C.byref(d), C.byref(g), C.byref(nb)) == 0
    assert nb.value == 256 * 4 * 4
    g.start[1] = 288
    d.k = 4                             # unsupported kernel size -> error code, no crash
    assert L.gpi_conv_blocks(C.byref(d), C.byref(g), C.byref(nb)) != 0


def test_vo_rows_host_query(lib):
    L = lib.lib()
    assert L.gpi_vo_rows(64, 8, lib.VO_CGR) == 81
    assert L.gpi_vo_rows(64, 8, lib.VO_FLUX) == 128
    assert L.gpi_vo_rows(64, 8, lib.VO_CGR | lib.VO_FLUX) == 209
    assert L.gpi_vo_rows(32, 4, lib.VO_CGR | lib.VO_FLUX) == 25 + 32
    assert L.gpi_vo_rows(64, 7, lib.VO_CGR) < 0        # fine grid must refine the coarse one
    assert L.gpi_vo_rows(64, 8, 0) < 0


def test_fom_workspace_host_query(lib):
    L = lib.lib()
    assert L.gpi_fom_workspace(64) == 2 * 64 * 65 + 6 * 65 * 63
    assert L.gpi_fom_workspace(1) < 0
    d = lib.FomDesc()                   # missing buffers -> argument error, nothing launched
    assert L.gpi_fom_solve(C.byref(d), None) != 0
    r = lib.RandomFieldDesc()
    assert L.gpi_random_field(C.byref(r), None) != 0


def test_random_subset_workspace_host_query(lib):
    L = lib.lib()
    nb = C.c_int64(0)
    assert L.gpi_random_subset_workspace(1 << 20, C.byref(nb)) == 0
    assert nb.value == 4 * ((1 << 16) + 64) + 8 * (1 << 20)
    assert L.gpi_random_subset_workspace(0, C.byref(nb)) != 0


def test_library_source_sha_matches_sources(lib):
    """gpi_source_sha() of the built library equals the sha1 of the sources next to it:
    a library built from other sources is refused at load."""
    so = C.CDLL(lib.LIB_PATH)
    so.gpi_source_sha.restype = C.c_char_p
    got = so.gpi_source_sha().decode()
    assert re.fullmatch(r'[0-9a-f]{40}', got), got
    assert got == lib.source_sha()
    assert lib.check_source_sha(so) == got


def test_stale_library_is_refused(lib, tmp_path, monkeypatch):
    """A touched source (copied tree with one byte appended to a kernel file) no longer matches the
    library's embedded sha: loading it raises, unless GPI_ALLOW_STALE_LIB=1."""
    import shutil
    pkg = os.path.join(ROOT, 'generative-physics-informed-pde_amd')
    src = tmp_path / 'csrc'
    shutil.copytree(os.path.join(pkg, 'csrc'), str(src), ignore=shutil.ignore_patterns('build*', '*.o'))
    inc = tmp_path / 'gpi.h'
    shutil.copy(HEADER, str(inc))
    monkeypatch.setattr(lib, 'SRC_DIR', str(src))
    monkeypatch.setattr(lib, 'INCLUDE_H', str(inc))
    so = C.CDLL(lib.LIB_PATH)
    so.gpi_source_sha.restype = C.c_char_p
    assert lib.check_source_sha(so)              # the unchanged copy matches
    with open(str(src / 'misc.hip'), 'a') as fh:
        fh.write('\n// touched\n')
    with pytest.raises(lib.NativeError, match='stale native library'):
        lib.check_source_sha(so)
    monkeypatch.setenv('GPI_ALLOW_STALE_LIB', '1')
    assert lib.check_source_sha(so)
