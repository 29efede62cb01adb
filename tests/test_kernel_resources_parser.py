"""tests/kernel_resources.py::parse on four remark blocks of a real compile of csrc/grdma_h2.hip (the flag's name at each
line's end is put back from kernel_resources.REMARKS): names of which one is a prefix of the other, a name behind the
links prefix, a block whose register and spill counts all differ, a block that lacks a field.  No compiler needed."""
import pytest

from tests.kernel_resources import FIELDS, REMARKS, parse, short_name

TEXT = """In file included from grpc-rdma_amd/csrc/grdma_h2.hip:31:
grpc-rdma_amd/csrc/grdma_h2_kernels.h:1121:1: remark: Function Name: _ZN12_GLOBAL__N_112k_h2_deframeEP19grdma_h2_parser_devPKhPK15grdma_slice_outmP14grdma_h2_eventmP23grdma_h2_deframe_result [@]
 1121 |                                                                   grdma_h2_deframe_result* res) {
      | ^
grpc-rdma_amd/csrc/grdma_h2_kernels.h:1121:1: remark:     TotalSGPRs: 106 [@]
grpc-rdma_amd/csrc/grdma_h2_kernels.h:1121:1: remark:     VGPRs: 142 [@]
grpc-rdma_amd/csrc/grdma_h2_kernels.h:1121:1: remark:     AGPRs: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_kernels.h:1121:1: remark:     ScratchSize [bytes/lane]: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_kernels.h:1121:1: remark:     Dynamic Stack: False [@]
grpc-rdma_amd/csrc/grdma_h2_kernels.h:1121:1: remark:     Occupancy [waves/SIMD]: 3 [@]
grpc-rdma_amd/csrc/grdma_h2_kernels.h:1121:1: remark:     SGPRs Spill: 57 [@]
grpc-rdma_amd/csrc/grdma_h2_kernels.h:1121:1: remark:     VGPRs Spill: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_kernels.h:1121:1: remark:     LDS Size [bytes/block]: 49224 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:339:1: remark: Function Name: _ZN12_GLOBAL__N_113k_h2_asm_copyEP7h2a_devPK8h2a_call [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:339:1: remark:     TotalSGPRs: 81 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:339:1: remark:     VGPRs: 89 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:339:1: remark:     AGPRs: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:339:1: remark:     ScratchSize [bytes/lane]: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:339:1: remark:     Dynamic Stack: False [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:339:1: remark:     Occupancy [waves/SIMD]: 5 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:339:1: remark:     SGPRs Spill: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:339:1: remark:     VGPRs Spill: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:339:1: remark:     LDS Size [bytes/block]: 3072 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:471:1: remark: Function Name: _ZN12_GLOBAL__N_119k_h2_asm_copy_linksEPKNS_8h2a_linkEj [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:471:1: remark:     TotalSGPRs: 80 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:471:1: remark:     VGPRs: 78 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:471:1: remark:     AGPRs: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:471:1: remark:     ScratchSize [bytes/lane]: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:471:1: remark:     Dynamic Stack: False [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:471:1: remark:     Occupancy [waves/SIMD]: 6 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:471:1: remark:     SGPRs Spill: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:471:1: remark:     VGPRs Spill: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_asm.h:471:1: remark:     LDS Size [bytes/block]: 5168 [@]
grpc-rdma_amd/csrc/grdma_h2_ctl.h:235:1: remark: Function Name: _ZN12_GLOBAL__N_119k_h2_links_ctl_lastEPKNS_10h2ctl_linkEj [@]
grpc-rdma_amd/csrc/grdma_h2_ctl.h:235:1: remark:     TotalSGPRs: 30 [@]
grpc-rdma_amd/csrc/grdma_h2_ctl.h:235:1: remark:     VGPRs: 12 [@]
grpc-rdma_amd/csrc/grdma_h2_ctl.h:235:1: remark:     AGPRs: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_ctl.h:235:1: remark:     ScratchSize [bytes/lane]: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_ctl.h:235:1: remark:     Dynamic Stack: False [@]
grpc-rdma_amd/csrc/grdma_h2_ctl.h:235:1: remark:     Occupancy [waves/SIMD]: 8 [@]
grpc-rdma_amd/csrc/grdma_h2_ctl.h:235:1: remark:     SGPRs Spill: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_ctl.h:235:1: remark:     VGPRs Spill: 0 [@]
grpc-rdma_amd/csrc/grdma_h2_ctl.h:235:1: remark:     LDS Size [bytes/block]: 8 [@]
""".replace("@", REMARKS)


def test_every_block_under_its_own_name_with_every_field():
    got = parse(TEXT)
    assert got == {
        "k_h2_deframe": {"sgprs": 106, "vgprs": 142, "agprs": 0, "scratch": 0, "occupancy": 3, "sspill": 57, "vspill": 0,
                         "lds": 49224},
        "k_h2_asm_copy": {"sgprs": 81, "vgprs": 89, "agprs": 0, "scratch": 0, "occupancy": 5, "sspill": 0, "vspill": 0,
                          "lds": 3072},
        "k_h2_asm_copy_links": {"sgprs": 80, "vgprs": 78, "agprs": 0, "scratch": 0, "occupancy": 6, "sspill": 0,
                                "vspill": 0, "lds": 5168},
        "k_h2_links_ctl_last": {"sgprs": 30, "vgprs": 12, "agprs": 0, "scratch": 0, "occupancy": 8, "sspill": 0,
                                "vspill": 0, "lds": 8},
    }
    # (the block that shows no field is taken for another: the four counts a careless pattern confuses all differ)
    d = got["k_h2_deframe"]
    assert len({d["vgprs"], d["vspill"], d["sspill"], d["sgprs"]}) == 4
    assert all(set(v) == set(FIELDS.values()) for v in got.values())


def test_the_name_is_cut_at_its_length_prefix():
    assert short_name("_ZN12_GLOBAL__N_113k_h2_asm_copyEP7h2a_devPK8h2a_call") == "k_h2_asm_copy"
    assert short_name("_ZN12_GLOBAL__N_122k_h2_asm_release_linksEPKNS_16h2a_link_releaseE") == "k_h2_asm_release_links"
    assert short_name("_Z14k_plan_pair_mwP9grdma_job") == "k_plan_pair_mw"    # (no scope, an `E`-free tail)
    assert short_name("k_plain_c_name") == "k_plain_c_name"
    with pytest.raises(ValueError):
        short_name("_ZN12_GLOBAL")


@pytest.mark.parametrize("label", sorted(FIELDS), ids=[FIELDS[x] for x in sorted(FIELDS)])
def test_a_block_that_lacks_a_field_raises(label):
    lines = TEXT.splitlines()
    at = [i for i, ln in enumerate(lines) if "remark:     %s: " % label in ln]
    assert len(at) == 4
    with pytest.raises(ValueError, match="k_h2_asm_copy_links"):
        parse("\n".join(lines[:at[2]] + lines[at[2] + 1:]))


def test_two_blocks_of_one_name_raise():
    with pytest.raises(ValueError, match="two remark blocks"):
        parse(TEXT + TEXT)
