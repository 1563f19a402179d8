"""tgx_verify_tree without a GPU: the built library exports the call, the header declares it with its node limit, the Python binding and the host engine's
backend table and C view know it, and the tree drafter is reachable through the host engine's configuration."""
import ctypes
import os
import re

from conftest import ROOT


def test_the_library_exports_verify_tree_and_the_binding_has_it():
    from tinygpt_amd import build
    from tinygpt_amd.ffi import ABI, Backend, Model
    lib = build.build_lib()
    assert "verify_tree" in ABI
    be = Backend(lib, "tgx_", required=["verify_tree", "abi_version"])      # AttributeError if the symbol is missing
    assert be.abi_version() == 3                                            # additive
    assert callable(getattr(Model, "verify_tree", None))
    # null pointers are refused before anything else is looked at (no context needed)
    assert be.verify_tree(None, 0, None, None, 0, None, None, None) == 1


def test_the_header_states_the_node_limit():
    src = open(os.path.join(ROOT, "include", "tgx.h")).read()
    m = re.search(r"#define\s+TGX_MAX_TREE_NODES\s+(\d+)", src)
    d = re.search(r"#define\s+TGX_MAX_DRAFT\s+(\d+)", src)
    assert m and d and int(m.group(1)) == int(d.group(1)) == 15             # root + nodes <= 16 positions of one pass


def test_the_host_engine_knows_the_call():
    from tinygpt_amd import build
    lib, cli = build.build_host()
    h = ctypes.CDLL(lib)
    assert hasattr(h, "tgxe_set_speculate_tree") and hasattr(h, "tgxe_spec_tree_passes")
    import subprocess
    out = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "--speculate-tree" in out.stdout + out.stderr
