"""tools/kernel_digest.py's normaliser and comparison on hand-written assembly (no compile, no GPU): a kernel's digest must
not depend on its symbol name, on its position in the file (the function number of its block labels), on comments or on
assembler directives — and must change with a single instruction."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "kernel_digest", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "kernel_digest.py"))
kd = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kd)


def _kernel(symbol, fn, last="v_add_f32_e32 v2, v1, v0"):
    """One kernel as the compiler writes it: type directive, label, body with a loop and a symbol reference, end marker."""
    return """
	.protected	{s}
	.globl	{s}
	.p2align	8
	.type	{s},@function
{s}:                                 ; @{s}
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 0                     ; a comment
	s_getpc_b64 s[2:3]
	s_add_u32 s2, s2, {s}.data@rel32@lo+4
.LBB{n}_1:                                ; =>This Inner Loop Header: Depth=1
	s_waitcnt lgkmcnt(0)

	v_mul_f32_e32 v0,   s0, v1
	s_cbranch_scc1 .LBB{n}_1
; %bb.2:
	{last}
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel {s}
		.amdhsa_next_free_vgpr 3
	.end_amdhsa_kernel
	.text
.Lfunc_end{n}:
	.size	{s}, .Lfunc_end{n}-{s}
""".format(s=symbol, n=fn, last=last)


OLD = _kernel("_Z13k_render_lensILb1EEvv", 7)
NEW = _kernel("_Z12k_render_recILb1ELi1024EEvv", 31)
OTHER = _kernel("_Z12k_render_recILb1ELi1024EEvv", 31, last="v_sub_f32_e32 v2, v1, v0")
RULES = [(r"_Z13k_render_lensI(.*)EEvv", r"_Z12k_render_recI\1ELi1024EEvv")]


def _names(names):  # (the listings below keep the mangled names: no demangler is needed)
    return list(names)


def test_normalise_keeps_instructions_and_block_labels_only():
    body = kd.normalise(kd.kernels(OLD)["_Z13k_render_lensILb1EEvv"])
    assert body == ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v1, 0", "s_getpc_b64 s[2:3]",
                    "s_add_u32 s2, s2, SYM.data@rel32@lo+4", ".LBB_1:", "s_waitcnt lgkmcnt(0)", "v_mul_f32_e32 v0, s0, v1",
                    "s_cbranch_scc1 .LBB_1", "v_add_f32_e32 v2, v1, v0", "s_endpgm"]


def test_same_body_under_another_name_and_numbering_compares_equal():
    a, b = kd.listing(OLD, _names), kd.listing(NEW, _names)
    assert [r[1] for r in a] == [9] and a[0][0] != b[0][0] and a[0][1:] == b[0][1:]
    assert kd.compare(a, b, RULES) == []
    assert len(kd.compare(a, b)) == 2  # without the map: one kernel only in each


def test_one_different_instruction_compares_unequal():
    a, b = kd.listing(OLD, _names), kd.listing(OTHER, _names)
    diffs = kd.compare(a, b, RULES)
    assert len(diffs) == 1 and diffs[0][0] == "_Z12k_render_recILb1ELi1024EEvv"
    assert kd.listing(NEW, _names)[0][2] != b[0][2]


def test_listing_covers_every_kernel_of_a_file_and_reads_back(tmp_path):
    rows = kd.listing(OLD + NEW, _names)
    assert len(rows) == 2 and rows[0][2] == rows[1][2]
    path = tmp_path / "digest.txt"
    path.write_text("".join("%-40s %6d %s\n" % r for r in rows))
    assert kd.read_listing(str(path)) == rows


def test_short_name():
    assert kd.short_name("void rtk::k_render_rec<true, false, true, 1, 1024, rtk::LensRec>(rtk::DevScene, rtk::RenderArgs, "
                         "rtk::LensRec, HIP_vector_type<float, 4u>*, unsigned long long*)") == "k_render_rec<true, false, true, 1, 1024, rtk::LensRec>"
    assert kd.short_name("rtk::(anonymous namespace)::k_fold(unsigned long long*)") == "rtk::k_fold"
