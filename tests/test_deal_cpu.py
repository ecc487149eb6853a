"""Dealt launches, the part that needs no GPU: the ticket -> (receiver tile, source part) map the kernel and the host share,
the auto rule of the "deal" hook, and the gfx950 ISA of the two dealt_kernel instantiations (hipcc cross-compiles).

A dealt launch runs the work of step_kernel<K, 16, scalar-cache route> with the item drawn from a ticket counter instead of
read off the block index (nbody_amd/csrc/kernels.hip dealt_kernel, step_tile.inc).  What must hold statically: every item
is handed out exactly once and nothing past the last one; the hot loop is the one the step kernels run; the ticket is the
only atomic, with its return value, and nothing else about memory ordering was added anywhere."""
import re

import pytest

import nbody_amd as nb
from isa_common import check_rsq_wait_states, compile_isa, functions, kernel_meta


@pytest.mark.parametrize("tiles,split", [(1, 16), (8192, 2), (8191, 3)])      # one tile; the headline; a prime tile count
def test_every_item_is_dealt_exactly_once_and_nothing_past_the_last(tiles, split):
    items = tiles * split
    seen = [nb.deal_item(t, tiles, split) for t in range(items)]
    assert None not in seen
    assert len(set(seen)) == items and set(seen) == {(x, y) for y in range(split) for x in range(tiles)}
    # the order of a (tiles, split) grid linearised x first: what keeps the access pattern of the classic launch
    assert seen[:3] == [(x % tiles, x // tiles) for x in range(3)] and seen[-1] == (tiles - 1, split - 1)
    for t in (items, items + 1, items + max(8, items // 32) - 1, 2 * items, 2 ** 32 - 1):
        assert nb.deal_item(t, tiles, split) is None, t
    assert nb.deal_item(0, 0, split) is None


def test_the_auto_rule_deals_launches_of_thirty_two_rounds_and_nothing_smaller():
    assert nb.plan_deal(1 << 20, 523884, 256)                    # the headline: 8 192 tiles x 2 parts = 32 rounds of 512
    for m in (1, 1000, 32768, 65536):
        assert not nb.plan_deal(65536, m, 256)                   # one round at most
    # below R = 32 rounds of resident workgroups (two per CU): off, whatever the split
    for n, m in ((131072, 65536), (262144, 131072), (524288, 262144), (786432, 393216)):
        plan = nb.plan_launch(n, m, 256)
        assert plan["workgroups"] < 32 * 512 and not nb.plan_deal(n, m, 256), (n, m, plan)
    # consistent with the launch plan for the same arguments: dealt exactly where the auto shape is one of the two
    # instantiated ones, no fused finish takes the step, and the items fill 32 rounds
    for n in (1000, 20000, 65536, 200000, 262144, 1 << 20, (1 << 20) + 77, 1 << 21):
        for m in (n // 2, n):
            for cus in (256, 128):
                plan = nb.plan_launch(n, m, cus)
                want = (plan["lanes"] <= 1 and plan["k"] in (1, 2) and plan["w"] == 16 and not plan["fused_finish"]
                        and plan["workgroups"] >= 32 * 2 * cus)
                assert nb.plan_deal(n, m, cus) == want, (n, m, cus, plan)


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("deal_isa"), "kernels.hip")


def test_dealt_kernels_run_the_step_kernels_loop_and_add_one_ticket(isa):
    fns = functions(isa)
    dealt = {n: b for n, b in fns.items() if "dealt_kernel" in n}
    assert sorted(re.search(r"dealt_kernelILi(\d+)ELi(\d+)EEEv", n).groups() for n in dealt) == [("1", "16"), ("2", "16")]
    assert not any("step_kernel" in n for n in dealt)              # test_isa.py's census of step_kernel stays what it was
    head = ["v_sub_f32", "v_sub_f32", "v_fma_f32", "v_fmac_f32"]
    tail = ["v_mul_f32", "v_mul_f32", "v_mul_f32", "v_fmac_f32", "v_fmac_f32"]
    single = head + ["s_setprio", "v_rsq_f32", "s_setprio"] + tail
    paired = head + head + ["s_setprio", "v_rsq_f32", "v_rsq_f32", "s_setprio"] + tail + tail
    for name, body in dealt.items():
        ops = [ins.split()[0] for ins in body]
        want = single if "ILi1E" in name else paired
        hits = sum(1 for i in range(len(ops) - len(want) + 1) if ops[i:i + len(want)] == want)
        assert hits >= 16, (name, hits)
        assert not any(op.endswith("_e64") for op in ops if op.startswith(("v_mul_f32", "v_fmac_f32", "v_rsq_f32", "v_sub_f32")))
        assert check_rsq_wait_states(name, body) >= 16
        # as many interactions as the classic kernel of the same shape unrolls
        twin = next(b for n, b in fns.items() if "step_kernel" + re.search(r"ILi\dELi16E", name).group(0) + "Li1ELb0E" in n)
        assert ops.count("v_rsq_f32") == [i.split()[0] for i in twin].count("v_rsq_f32")
        # the sources still arrive through the scalar cache although an atomic precedes the loop
        assert sum(op.startswith("s_load_dwordx16") for op in ops) >= 2 and sum(op.startswith("s_load_dwordx8") for op in ops) >= 2
        text = "\n".join(body)
        atom = [x for x in body if x.startswith("global_atomic")]
        assert len(atom) == 1 and atom[0].startswith("global_atomic_add") and "sc0" in atom[0], (name, atom)   # with return
        assert "buffer_wbl2" not in text and "buffer_inv" not in text, name
        # the parts are plain stores, as in the unfused step kernel: no sc1 access to anything 8 bytes wide
        assert not re.search(r"global_(load|store)_dwordx2 .* sc1", text), name
    meta = {n: (scratch, vgpr) for n, scratch, _, vgpr in kernel_meta(isa) if "dealt_kernel" in n}
    assert len(meta) == 2
    for name, (scratch, vgpr) in meta.items():
        assert vgpr <= 48 and scratch == 0, (name, vgpr, scratch)


def test_no_other_kernel_gained_an_atomic(isa):
    """Atomics in kernels.hip: the six fused-finish step kernels' tile tickets, the two dealt kernels' counter, nothing else."""
    with_atomic = {n for n, b in functions(isa).items() if any("_atomic" in ins for ins in b)}
    fused = {n for n in with_atomic if "step_kernel" in n and re.search(r"Lb1EEEv", n)}
    dealt = {n for n in with_atomic if "dealt_kernel" in n}
    assert len(fused) == 6 and len(dealt) == 2 and with_atomic == fused | dealt, sorted(with_atomic - fused - dealt)
