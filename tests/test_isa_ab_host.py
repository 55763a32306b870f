"""tools/isa_ab.py on synthetic assembly: what may differ between two builds of the same kernel (its mangled name, label
numbers, comments, the __hip_cuid symbol) compares equal; an instruction, a descriptor field or a missing kernel does not."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_ab", os.path.join(ROOT, "tools", "isa_ab.py"))
isa_ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_ab)


def _kernel(name, fn, add="v_add_u32_e32 v1, v0, v0", vgpr=42, note="one"):
    return """
	.section	.text.{n},"axG",@progbits,{n},comdat
	.globl	{n} ; -- Begin function {n}
	.p2align	8
	.type	{n},@function
{n}:                                    ; @{n}
; %bb.0:                                ; {note}
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_cbranch_scc1 .LBB{f}_2
.LBB{f}_1:                              ; =>This Inner Loop Header: Depth=1
	{add}
	s_cbranch_scc0 .LBB{f}_1
.LBB{f}_2:
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel {n}
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_next_free_vgpr {v}
	.end_amdhsa_kernel
	.section	.text.{n},"axG",@progbits,{n},comdat
.Lfunc_end{f}:
	.size	{n}, .Lfunc_end{f}-{n}
""".format(n=name, f=fn, add=add, v=vgpr, note=note)


def _file(kernels, cuid="0123abcd"):
    return "\t.text\n" + "".join(kernels) + "\t.type\t__hip_cuid_%s,@object\n__hip_cuid_%s:\n\t.byte 0\n" % (cuid, cuid)


A = _file([_kernel("_Z1aILb1ELi3EEv", 0), _kernel("_Z1bv", 1, add="v_mul_f32_e32 v1, v0, v0")])


def _same(x, y):
    return isa_ab.compare(isa_ab.kernels(x), isa_ab.kernels(y))[1]


def test_names_labels_comments_compare_equal():
    b = _file([_kernel("_Z1bv", 7, add="v_mul_f32_e32 v1, v0, v0", note="other"),           # other order, other numbers
               _kernel("_Z1aI7VariantILb1ELi3EEEv", 3, note="two")], cuid="ffff0000")
    ka = isa_ab.kernels(A)
    assert [k.name for k in ka] == ["_Z1aILb1ELi3EEv", "_Z1bv"] and [k.n_instr for k in ka] == [5, 5]
    report, ok = isa_ab.compare(ka, isa_ab.kernels(b))
    assert ok and len(report) == 2 and all(ln.startswith("identical") for ln in report)
    assert "_Z1aILb1ELi3EEv  ==  _Z1aI7VariantILb1ELi3EEEv" in report[0]


def test_changed_instruction_differs():
    b = _file([_kernel("_Z1aILb1ELi3EEv", 0, add="v_add_u32_e32 v1, v0, v1"), _kernel("_Z1bv", 1, add="v_mul_f32_e32 v1, v0, v0")])
    report, ok = isa_ab.compare(isa_ab.kernels(A), isa_ab.kernels(b))
    assert not ok
    assert [ln.split()[0] for ln in report] == ["identical", "DIFFERS"]


def test_differs_says_which_descriptor_lines_and_opcode_counts():
    b = _file([_kernel("_Z1aILb1ELi3EEv", 0, add="v_add_u32_e32 v1, v0, v1\n\tds_read_b32 v2, v1\n\ts_nop 0", vgpr=43),
               _kernel("_Z1bv", 1, add="v_mul_f32_e32 v1, v0, v0")])
    report, ok = isa_ab.compare(isa_ab.kernels(A), isa_ab.kernels(b))
    assert not ok and len(report) == 2
    more = report[1].split("\n")[1:]
    assert [ln.strip() for ln in more] == ["descriptor: .amdhsa_next_free_vgpr 42 -> 43", "opcodes: ds_read_b32 0 -> 1"]   # (no s_nop)
    same = _file([_kernel("_Z1aILb1ELi3EEv", 0, add="s_nop 0"), _kernel("_Z1bv", 1, add="v_mul_f32_e32 v1, v0, v0")])
    more = isa_ab.compare(isa_ab.kernels(A), isa_ab.kernels(same))[0][1].split("\n")[1:]
    assert [ln.strip() for ln in more] == ["descriptor: the same", "opcodes: v_add_u32_e32 1 -> 0"]


def test_changed_descriptor_field_differs():
    assert not _same(A, _file([_kernel("_Z1aILb1ELi3EEv", 0, vgpr=43), _kernel("_Z1bv", 1, add="v_mul_f32_e32 v1, v0, v0")]))


def test_missing_kernel_differs():
    b = _file([_kernel("_Z1aILb1ELi3EEv", 0)])
    report, ok = isa_ab.compare(isa_ab.kernels(A), isa_ab.kernels(b))
    assert not ok and any("(missing)" in ln for ln in report) and "kernel counts differ: 2 against 1" in report[-1]
    assert not _same(b, A)
    # two copies of one body are two kernels: a multiset, not a set
    assert not _same(_file([_kernel("_Z1xv", 0), _kernel("_Z1yv", 1)]), _file([_kernel("_Z1xv", 0)]))


def test_names_are_compared_as_multisets_of_demangled_names():
    """--names: equal bodies under other names (which the body comparison accepts) differ; order does not"""
    a = isa_ab.demangled(["_Z1aILb1ELi3EEvv", "_Z1bv"])
    assert a == ["void a<true, 3>()", "b()"]
    report, ok = isa_ab.compare_names(a, a[::-1])
    assert ok and report == ["names: the same 2 demangled kernel names"]
    report, ok = isa_ab.compare_names(a, isa_ab.demangled(["_Z1aI7VariantILb1ELi3EEEvv", "_Z1bv"]))
    assert not ok and len(report) == 2 and "only in A" in report[0] and "only in B" in report[1]
    assert not isa_ab.compare_names(a, a + a[:1])[1]
