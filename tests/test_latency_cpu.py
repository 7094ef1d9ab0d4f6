"""The latency schedule's public surface and build products, without a GPU: the rfd_config layout, rfd_create's validation of
`schedule` (done before the device probe), and the DESIGN.md section 5 hazard rules on kernels_splitk.o (the same checks
tests/test_build_cpu.py applies to the other objects)."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "rs-face-detection_amd", "build")
LLVM = "/opt/rocm/lib/llvm/bin"
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_check  # noqa: E402
from test_build_cpu import _kernel_notes  # noqa: E402

_needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="LLVM tools not installed")


def test_config_layout_and_schedule_validation(rfd):
    cfg = rfd.rfd_config()
    assert ctypes.sizeof(cfg) == 64
    assert rfd.rfd_config.schedule.offset == 44 and rfd.rfd_config.precision.offset == 40
    assert (rfd.SCHEDULE_THROUGHPUT, rfd.SCHEDULE_LATENCY) == (0, 1) and rfd.LATENCY_MAX_BATCH >= 2
    L = rfd.load_library()
    L.rfd_config_default(ctypes.byref(cfg))
    assert cfg.schedule == rfd.SCHEDULE_THROUGHPUT
    ctx = ctypes.c_void_p()
    cfg.schedule = 7
    assert L.rfd_create(ctypes.byref(cfg), ctypes.byref(ctx)) == rfd.RFD_ERR_INVALID_ARG
    assert b"schedule" in L.rfd_last_error()
    cfg.schedule = -1
    assert L.rfd_create(ctypes.byref(cfg), ctypes.byref(ctx)) == rfd.RFD_ERR_INVALID_ARG
    cfg.schedule = rfd.SCHEDULE_LATENCY
    cfg.precision = rfd.PRECISION_F32
    assert L.rfd_create(ctypes.byref(cfg), ctypes.byref(ctx)) == rfd.RFD_ERR_INVALID_ARG
    assert b"latency" in L.rfd_last_error()
    # a valid latency configuration passes validation: it fails only for want of a device (or succeeds where there is one)
    cfg.precision = rfd.PRECISION_BF16
    st = L.rfd_create(ctypes.byref(cfg), ctypes.byref(ctx))
    if torch.cuda.is_available():
        assert st == rfd.RFD_OK
        out = rfd.rfd_config()
        assert L.rfd_get_config(ctx, ctypes.byref(out)) == rfd.RFD_OK and out.schedule == rfd.SCHEDULE_LATENCY
        L.rfd_destroy(ctx)
    else:
        assert st == rfd.RFD_ERR_NO_DEVICE


def test_latency_max_batch_matches_the_header(rfd):
    import re
    with open(os.path.join(ROOT, "include", "rfd.h")) as f:
        m = re.search(r"#define\s+RFD_LATENCY_MAX_BATCH\s+(\d+)", f.read())
    assert m and int(m.group(1)) == rfd.LATENCY_MAX_BATCH


@pytest.fixture(scope="module")
def splitk(tmp_path_factory):
    obj = os.path.join(BUILD, "kernels_splitk.o")
    assert os.path.exists(obj), "run rs-face-detection_amd/build.sh (or __graft_entry__.build()) first"
    tmp = str(tmp_path_factory.mktemp("isa_splitk"))
    return obj, tmp, isa_check.disassemble(obj, tmp)


@_needs_llvm
def test_splitk_kernels_do_not_spill(splitk):
    obj, tmp, _ = splitk
    notes = _kernel_notes(obj, tmp)
    assert len(notes) >= 1
    for name, scratch, vsp, ssp, vgpr in notes:
        assert "conv_splitk_kernel" in name
        assert scratch == 0 and vsp == 0 and ssp == 0, "%s: %d bytes of scratch, %d VGPR / %d SGPR spills (vgpr_count %d)" % (name, scratch, vsp, ssp, vgpr)


@_needs_llvm
def test_splitk_kernels_obey_the_hazard_rules(splitk):
    _, _, kernels = splitk
    assert len(kernels) >= 1
    for name, ins in kernels.items():
        assert isa_check.uses_lds_dma(ins), "%s does not stage by LDS-DMA" % name
        assert isa_check.has_instr(ins, "v_mfma_f32_16x16x32_bf16"), name
        bad = isa_check.pending_lds_reads_at_barriers(ins)
        assert not bad, "%s: LDS reads may be in flight at s_barrier %s" % (name, bad)
        assert not isa_check.counted_vmcnt_with_store_in_flight(ins), name
        assert not isa_check.counted_vmcnt_waits(ins), "%s: a counted vmcnt publishes LDS-DMA data (every wait drains)" % name
        bad = isa_check.ds_read_b128_under_partial_exec(ins)
        assert not bad, "%s: ds_read_b128 under a possibly partial EXEC at %s" % (name, bad[:8])
