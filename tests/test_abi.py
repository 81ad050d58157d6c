"""C-ABI boundary checks that need no GPU: the library loads and exports every symbol the
header declares (no compute calls)."""
import ast
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fish-speech_amd", "fishmi", "libfishmi.so")


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "fishmi.h")).read()
    return sorted(set(re.findall(r"\b(fm_[a-z_0-9]+)\s*\(", src)))


def test_header_matches_python_binding_list():
    from fishmi import native

    assert sorted(native.ABI_SYMBOLS) == _header_symbols()


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfishmi.so not built (run __graft_entry__.build())")
def test_library_exports_every_header_symbol():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = set(re.findall(r" T (fm_[a-z_0-9]+)", out))
    missing = [s for s in _header_symbols() if s not in exported]
    assert not missing, missing


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfishmi.so not built")
def test_library_built_from_this_tree():
    """Build provenance: the loaded libfishmi.so carries the hash of the sources it was compiled
    from (Makefile HASHED), and it equals the hash of the sources in this tree -- a stale prebuilt
    library cannot pass (native.lib() refuses it)."""
    import ctypes

    from fishmi import native

    L = ctypes.CDLL(native.LIB_PATH)
    L.fm_source_hash.restype = ctypes.c_char_p
    built = L.fm_source_hash().decode()
    assert len(built) == 16 and built == native.tree_source_hash()


def test_library_loads_without_gpu():
    from fishmi import native

    L = native.lib()
    assert L.fm_device_count() >= 0
    for s in _header_symbols():
        assert hasattr(L, s)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfishmi.so not built")
def test_library_maps_torch_hip_runtime_first():
    """A fresh process that loads fishmi first must end up on torch's libamdhip64 (one HIP runtime
    per process; the other order leaves torch with "No HIP GPUs are available" on the box)."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from fishmi import native; native.lib()\n"
            "maps = [l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l]\n"
            "print(sorted(set(maps)))\n") % os.path.join(ROOT, "fish-speech_amd")
    out = subprocess.check_output(["python3", "-c", code], text=True, timeout=300)
    paths = ast.literal_eval(out.strip().splitlines()[-1])
    assert len(paths) == 1 and "/torch/lib/" in paths[0], paths


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfishmi.so not built")
def test_host_rope_table_matches_reference(golden):
    """The bf16 cos/sin table the library builds on the host (fm_rope_table, no device) equals the
    reference's precompute_freqs_cis (llama.py:1003-1022) bit for bit, both goldens of ops.npz."""
    import numpy as np

    from fishmi import ops

    g = golden("ops.npz")
    t = ops.rope_table(64, 32, 10000)
    np.testing.assert_array_equal(t, g["rope_table"].reshape(t.shape))
    t2 = ops.rope_table(4096, 128, 1000000)[::97]
    np.testing.assert_array_equal(t2, g["rope_table_big"].reshape(t2.shape))


# fm_tune's keys as the hand-written if-chain accepted them before the knob table (fm_tune_table.h)
# replaced it, written out from that chain: key -> (an accepted value that is not the default, values the
# chain rejected).  Not derived from the table, so it pins the table to the old behaviour.
_BOOL_KNOBS = """gemv_nt sampler_fast prefill_attn prefix_vec prompt_qkv_slab prompt_unroll prompt_fin prompt_swiglu
    prompt_skinny prompt_gemm conv2 conv_splitk codec_norm codec_rope codec_swiglu codec_fuse resunit_enc resunit_384
    attn_wo batched_fused_attn ksb_balance attn3 attn_fd gemv_chain bs_qkv_slab fast_tail fkv_prefetch kv_prefetch
    bstream bs_xfirst bs_vec_epi fin8 int4_stream bstream_q8 fw_prio fw_cheap fattn_wo fattn_ilp sampler_kth row_copies
    rmsnorm_block""".split()
_VALUE_KNOBS = {
    "gemv_u": (4, [3, 0, 16]), "attn_cap": (64, [8, 24, -16]), "prompt_skinny_blocks": (1, [0, -1]),
    "prompt_ks_tiles": (1, [0]), "prompt_ks_max": (2, [3, 0, 16]), "resunit_cfg": (2, [3, -1]), "gemv_wpb": (8, [6, 16]),
    "ksb_blocks": (64, [0]), "attn_cap_batched": (0, [8, 24]), "linear_u32": (8, [6, 0]), "linear_fill": (1024, [-1]),
    "fd_min": (16, [0, 8, 24]), "chain_max": (2, [5, 1]), "chain_sleep": (16, [2, 0]), "fd_nw": (16, [5, 2, 32]),
    "fin_ksb": (8, [9, -1]), "fd_nw_batched": (8, [5, 0]), "fd_min16": (16, [0, 24]), "fd_min_batched": (64, [8, 0]),
    "gemv_dummy": (0, [3, -1]), "bs_dummy": (1, [3, -1]), "bstream_kparts": (8, [3, 16]), "bstream_nw": (16, [17, -1]),
    "bsacc_kparts": (4, [16, 3]), "q_u": (16, [3, 1, 32]), "fin_split": (16, [17, -1]), "fw_delay": (1000, [1001, -1]),
    "row_qkv_rp": (16, [2, 32]), "rowgemv_q4": (0, [32, -1]), "rowgemv": (27, [128, -1]),
    "bstream_acc": (2, []), "bstream_chain": (2, []),  # stored as given, any value
}


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfishmi.so not built")
def test_tune_keys_values_and_getter():
    """fm_tune / fm_tune_get over every key of the old chain but "debug_ts" (which allocates on the
    device): the value in force reads back and is accepted, every value the chain rejected still
    fails, a set reads back (bools as value != 0), and the old value is put back; unknown keys fail."""
    from fishmi import native

    cases = {k: (None, []) for k in _BOOL_KNOBS}
    cases.update(_VALUE_KNOBS)
    assert len(cases) == 73
    for key, (other, rejected) in cases.items():
        old = native.tune_get(key)
        native.tune(key, old)
        assert native.tune_get(key) == old
        try:
            for bad in rejected:
                with pytest.raises(native.FishMIError):
                    native.tune(key, bad)
                assert native.tune_get(key) == old, (key, bad)
            if other is None:
                for v, want in ((1 - old, 1 - old), (5, 1), (0, 0)):
                    native.tune(key, v)
                    assert native.tune_get(key) == want, (key, v)
            else:
                native.tune(key, other)
                assert native.tune_get(key) == other, key
        finally:
            native.tune(key, old)
        assert native.tune_get(key) == old
    for f in (lambda: native.tune("no_such_knob", 1), lambda: native.tune_get("no_such_knob")):
        with pytest.raises(native.FishMIError) as e:
            f()
        assert e.value.code == -1  # FM_ERR_ARG


def test_rowgemv_default_is_the_documented_one():
    """The default of "rowgemv" (include/fishmi.h: 123) in a process no test has tuned yet."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from fishmi import native; print(native.tune_get('rowgemv'))\n") % os.path.join(ROOT, "fish-speech_amd")
    env = {k: v for k, v in os.environ.items() if k != "FISHMI_TUNE"}
    assert subprocess.check_output(["python3", "-c", code], text=True, timeout=300, env=env).split()[-1] == "123"
