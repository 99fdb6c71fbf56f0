"""tools/kernel_streams.py decides whether a refactor left a kernel's device code what it was: it must call
two listings EQUAL when only local label numbers, comments and directives moved, DIFF when an instruction moved or changed,
tell a changed descriptor from changed instructions, and pair renamed kernels only when told to.  Hand-written assembly,
nothing compiled, no GPU."""
import importlib.util
import os

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_spec = importlib.util.spec_from_file_location("kernel_streams", os.path.join(ROOT, "tools", "kernel_streams.py"))
ks = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ks)

BASE = """\
	.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
	.globl	kern_a                          ; -- Begin function kern_a
	.p2align	8
	.type	kern_a,@function
kern_a:                                 ; @kern_a
; %bb.0:
	s_load_dwordx2 s[4:5], s[0:1], 0x0
	v_mov_b32_e32 v1, 0
	s_cbranch_scc1 .LBB0_2
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	v_add_u32_e32 v1, 1, v1
	v_add_f32_e32 v2, v1, v0
	s_cbranch_execnz .LBB0_1
.LBB0_2:
	global_store_dword v0, v2, s[4:5]
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel kern_a
		.amdhsa_group_segment_fixed_size 208
		.amdhsa_next_free_vgpr 3
		.amdhsa_next_free_sgpr 6
	.end_amdhsa_kernel
	.text
.Lfunc_end0:
	.size	kern_a, .Lfunc_end0-kern_a
	.set kern_a.num_vgpr, 3
; Kernel info:
; NumVgprs: 3
; Occupancy: 8
	.amdgpu_metadata
---
amdhsa.kernels:
  - .args:
      - .offset:         0
        .size:           8
    .group_segment_fixed_size: 208
    .name:           kern_a
    .sgpr_spill_count: 0
    .symbol:         kern_a.kd
    .vgpr_count:     3
amdhsa.version:
  - 1
  - 2
...
"""
# another compile of the same code: the function is the file's fourth, its blocks are numbered otherwise, a remark changed,
# an alignment directive sits in the loop
RENUMBERED = (BASE.replace(".LBB0_1", ".LBB3_7").replace(".LBB0_2", ".LBB3_9").replace("Lfunc_end0", "Lfunc_end3")
              .replace("; =>This Inner Loop Header: Depth=1", "; =>another remark")
              .replace("\tv_add_u32_e32 v1, 1, v1\n", "\t.p2align	4\n\n\tv_add_u32_e32 v1, 1, v1 ; a comment\n"))
SWAPPED = BASE.replace("\tv_add_u32_e32 v1, 1, v1\n\tv_add_f32_e32 v2, v1, v0\n", "\tv_add_f32_e32 v2, v1, v0\n\tv_add_u32_e32 v1, 1, v1\n")
REGISTER = BASE.replace("v_add_f32_e32 v2, v1, v0", "v_add_f32_e32 v2, v1, v3")
RETARGETED = BASE.replace("s_cbranch_scc1 .LBB0_2", "s_cbranch_scc1 .LBB0_1")
DESCRIPTOR = BASE.replace(".amdhsa_next_free_sgpr 6", ".amdhsa_next_free_sgpr 14")
SPILLS = BASE.replace(".sgpr_spill_count: 0", ".sgpr_spill_count: 21")
RENAMED = BASE.replace("kern_a", "kern_b")


def run(tmp_path, capsys, old, new, *opts):
    (tmp_path / "old.s").write_text(old)
    (tmp_path / "new.s").write_text(new)
    rc = ks.main([str(tmp_path / "old.s"), str(tmp_path / "new.s"), *opts])
    return rc, capsys.readouterr().out


def test_parse_takes_instructions_and_metadata_apart():
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".s") as f:
        f.write(BASE)
        f.flush()
        insts, meta = ks.kernels(f.name)["kern_a"]
    assert insts == ["s_load_dwordx2 s[4:5], s[0:1], 0x0", "v_mov_b32_e32 v1, 0", "s_cbranch_scc1 .L0", ".L1:", "v_add_u32_e32 v1, 1, v1",
                     "v_add_f32_e32 v2, v1, v0", "s_cbranch_execnz .L1", ".L0:", "global_store_dword v0, v2, s[4:5]", "s_endpgm"]
    for line in (".amdhsa_kernel @", ".amdhsa_next_free_sgpr 6", ".set @.num_vgpr, 3", "; Occupancy: 8", ".vgpr_count: 3", ".symbol: @.kd",
                 "- .offset: 0", ".size: 8"):
        assert line in meta, (line, meta)
    assert not any("amdhsa.version" in l or l == "- 1" for l in meta)


def test_renumbered_labels_comments_and_directives_are_equal(tmp_path, capsys):
    rc, out = run(tmp_path, capsys, BASE, RENUMBERED)
    assert rc == 0 and out == "kern_a: instructions 8 / 8 EQUAL, metadata EQUAL\n"


def test_swapped_pair_of_instructions_differs(tmp_path, capsys):
    rc, out = run(tmp_path, capsys, BASE, SWAPPED, "--diff", "1")
    assert rc == 1 and "instructions 8 / 8 DIFF, metadata EQUAL" in out
    assert "old: v_add_u32_e32 v1, 1, v1" in out and "new: v_add_f32_e32 v2, v1, v0" in out


def test_changed_register_differs(tmp_path, capsys):
    rc, out = run(tmp_path, capsys, BASE, REGISTER)
    assert rc == 1 and "instructions 8 / 8 DIFF, metadata EQUAL" in out


def test_branch_to_another_label_differs(tmp_path, capsys):
    rc, out = run(tmp_path, capsys, BASE, RETARGETED)
    assert rc == 1 and "instructions 8 / 8 DIFF" in out


def test_changed_descriptor_differs_on_the_metadata_alone(tmp_path, capsys):
    for changed in (DESCRIPTOR, SPILLS):
        rc, out = run(tmp_path, capsys, BASE, changed)
        assert rc == 1 and out == "kern_a: instructions 8 / 8 EQUAL, metadata DIFF\n"


def test_map_pairs_renamed_kernels(tmp_path, capsys):
    rc, out = run(tmp_path, capsys, BASE, RENAMED)
    assert rc == 1 and out.count("UNPAIRED") == 2 and "kern_a" in out and "kern_b" in out
    rc, out = run(tmp_path, capsys, BASE, RENAMED, "--map", "kern_a=kern_b")
    assert rc == 0 and out == "kern_a -> kern_b: instructions 8 / 8 EQUAL, metadata EQUAL\n"
    rc, out = run(tmp_path, capsys, BASE, RENAMED.replace("v_mov_b32_e32 v1, 0", "v_mov_b32_e32 v1, 1"), "--map", "kern_a=kern_b")
    assert rc == 1 and "DIFF" in out
