#!/usr/bin/env python3
"""Build gate for the hand-scheduled kernels (called by opencl_raytracer_amd/csrc/Makefile).

Reads hipcc's `-Rpass-analysis=kernel-resource-usage` remarks for kernels.hip and fails
the build when a hot kernel would spill vector registers to scratch or run at fewer than
8 waves per SIMD: walk_collect (kernels.hip) hard-codes its scratch registers inside
kernels pinned to a 64-VGPR budget (`amdgpu_waves_per_eu(8, 8)`), so growth in live VGPRs
would otherwise turn into silent scratch traffic in the hottest loop.

    check_kernel_resources.py <remarks.txt> [--table out.txt] [--isa kernels.s] [--report-only]

Hot kernels (must have VGPR spill 0, scratch 0, occupancy 8): the default path, i.e.
primary_kernel, its posed form primary_posed_kernel (a host with a camera
pose: the same pass, eye and basis read from the launch constants) and ao_kernel<1, ..> (1 = UNIFORM).  The build
fails, too, when one of the two primary kernels is not found in the remarks at all: the kernels are matched by the prefix
of their demangled names, and a gate that matches nothing guards nothing.  The RANDOM
mode (ao_kernel<2, ..>, outside the bit-exact contract) must keep the occupancy; its
spills are reported, not fatal.  The ray-query kernels (query_kernel<true> / <false>, query_key_kernel,
query_scatter_kernel, query_scan_kernel: kernels/query.hip.h; and the kernels beside them: multi-hit, ambient-occlusion
queries, directional occlusion queries, frame layers and multi-view rendering) must be present, with VGPR spill 0 and scratch 0
(the directional kernels: no SGPR spill either, and their walk, ao_mask_kernel, at 8 waves per SIMD); they do
not use walk_collect's fixed registers (their walk is the exact form, plain C++ around one scalar load per node), so no
occupancy is pinned for them -- a spill there would still be memory traffic on every node of every query.  SGPR spills go to VGPR lanes (v_writelane / v_readlane), not
to memory -- but those are vector instructions, the very resource the walk is bound by, so
WHERE they land matters: with `--isa` (the device assembly of the same translation unit,
`hipcc --cuda-device-only -S`) the tool locates every lane operation of the hot kernels by
loop depth and fails the build when one sits inside the hand-scheduled node loop (the asm
blocks between .Lw_miss_a and .Lw_out), when the loop around it -- one turn per leaf stop or
batch -- holds more than LANE_OPS_PER_WALK_TURN of them, or when the per-packet code holds more
than LANE_OPS_PER_PACKET.  With `--isa` the table also lists, for the ambient-occlusion kernels, the static
instruction counts by class (VALU, SALU, SMEM, branch, wait, LDS, VMEM) of the node loop's labelled
stretches, of the code between the loop around it and the block, and by loop depth (scalar_side_by_place):
what profiles/ao_scalar_side_notes.md multiplies by event counts.  A report; nothing fails on it.
"""
import re
import subprocess
import sys

LANE_OPS_PER_WALK_TURN = 10  # v_readlane / v_writelane per turn of the loop around walk_collect, i.e. per leaf stop or batch (measured: 6 primary;
                             # 9 AO: four in the batch block, five single reloads on paths that exclude each other)
LANE_OPS_PER_PACKET = 40     # ... in the per-packet code around that loop (measured: 38 of ~700 vector instructions)
# ... and for the posed form of the primary pass (primary_posed_kernel), which holds more launch constants around the walk
POSED_LANE_OPS_PER_WALK_TURN = 4  # (measured: 2 -- the eye is read again at every leaf stop instead of being held, kernels/primary.hip.h)
POSED_LANE_OPS_PER_PACKET = 8     # (measured: 5 of ~700 vector instructions)
HOT_PRIMARY = ("primary_kernel", "primary_posed_kernel")

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
          "VGPRs Spill", "LDS Size [bytes/block]")


def demangle(name: str) -> str:
    try:
        out = subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return name
    return re.sub(r"\(.*", "", out)  # drop the parameter list


def parse(text: str):
    kernels, current = [], None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            current = {"name": demangle(m.group(1))}
            kernels.append(current)
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\S+) \[-Rpass-analysis", line)
        if m and current is not None and m.group(1).strip() in FIELDS:
            current[m.group(1).strip()] = m.group(2)
    return kernels


def lane_ops_by_place(isa_text: str):
    """Per kernel of the device assembly: where its v_readlane / v_writelane (SGPR spill traffic) sit.  Returns
    {demangled name: {"total", "in_node_loop", "walk_turn", "per_packet", "depths": {depth: count}}}."""
    lines = isa_text.split("\n")
    out, name, start = {}, None, 0
    for i, line in enumerate(lines):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, start = m.group(1), i
        if line.startswith(".Lfunc_end") and name is not None:
            body = lines[start:i]
            regions, begin = [], None  # the hand-scheduled node loops: .Lw_miss_a_N ... .Lw_out_N
            for j, text in enumerate(body):
                if re.search(r"\.Lw_miss_a_\d+:", text):
                    begin = j
                if re.search(r"\.Lw_out_\d+:", text) and begin is not None:
                    regions.append((begin, j))
                    begin = None
            if regions:
                # loop depth of a line = the depth noted at the last basic-block label before it
                # ("in Loop: Header=... Depth=N" on the label's own line or on a "; %bb.N:" comment; a loop header lists
                # its parents first, over several comment lines, and says "This Inner Loop Header: Depth=N" /
                # "This Loop Header: Depth=N" last: that one counts)
                depth, depths = 0, []
                for j, text in enumerate(body):
                    m = re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)(.*)", text)
                    if m:
                        note, k = m.group(2), j + 1
                        while k < len(body) and re.match(r"^\s+;", body[k]):  # the comment's continuation lines
                            note += body[k]
                            k += 1
                        own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", note)
                        inside = re.search(r"in Loop: Header=\S+ Depth=(\d+)", note)
                        depth = int(own.group(1)) if own else int(inside.group(1)) if inside else 0
                    depths.append(depth)
                lane = [j for j, text in enumerate(body) if "v_writelane" in text or "v_readlane" in text]
                walk_depth = max(depths[a] for a, _ in regions)  # the loop that holds the asm blocks
                by_depth = {}
                for j in lane:
                    by_depth[depths[j]] = by_depth.get(depths[j], 0) + 1
                out[demangle(name)] = {
                    "total": len(lane), "in_node_loop": sum(1 for j in lane if any(a <= j <= b for a, b in regions)),
                    "walk_turn": by_depth.get(walk_depth, 0), "per_packet": by_depth.get(walk_depth - 1, 0),
                    "depths": dict(sorted(by_depth.items())), "walk_depth": walk_depth}
            name = None
    return out


CLASSES = ("VALU", "SALU", "SMEM", "branch", "wait", "LDS", "VMEM")


def instruction_class(text: str):
    """The class of one line of device assembly, None for labels, comments and directives.  SALU: scalar instructions other
    than loads, branches and waits -- the classes of SQ_INSTS_SALU, SQ_INSTS_SMEM and SQ_INSTS_BRANCH."""
    m = re.match(r"^\s+([a-z_0-9]+)", text)
    if not m:
        return None
    op = m.group(1)
    if op.startswith(("s_load_", "s_buffer_load_", "s_memrealtime", "s_memtime")):
        return "SMEM"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_endpgm", "s_call")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier")):
        return "wait"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith("v_"):
        return "VALU"
    return None


def count_classes(lines):
    out = dict.fromkeys(CLASSES, 0)
    for text in lines:
        c = instruction_class(text)
        if c:
            out[c] += 1
    return out


def class_row(name, counts):
    return f"  {name:40s} " + " ".join(f"{counts[c]:6d}" for c in CLASSES)


def scalar_side_by_place(isa_text: str):
    """For the kernels that hold the ANY-HIT form of the node loop (ao_kernel<..>, one block each): static instruction counts
    by class
      - per labelled stretch of the hand-scheduled block (.Lw_miss_a = the pair's load, its checks and the test of `a`;
        .Lw_next_b = the test of `b` and, behind it, the descend; .Lw_next_a / .Lw_miss_b = the steps to the next pair;
        .Lw_leaf_a / .Lw_leaf_b = a leaf some lane hit, up to the append's end; .Lw_now / .Lw_full / .Lw_over = the exits),
      - from the header of the loop around the block to ;;#ASMSTART, and from ;;#ASMEND on while the instructions stay
        scalar (the dispatch on the block's status, along the text: the fall-through path),
      - by loop depth outside the block: the block's own depth is the turn around it (dispatch, the leaf tested on the spot,
        a full batch), one above it the packet (its set-up, the flush of a partial batch), two above it the job.
    Multiplied by the event counts of an instrumented run (tools/analysis/stamps_run.py) these give the per-launch table of
    profiles/ao_scalar_side_notes.md.  Returns the report's lines."""
    lines = isa_text.split("\n")
    report, name, start = [], None, 0
    for i, line in enumerate(lines):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, start = m.group(1), i
        if not (line.startswith(".Lfunc_end") and name is not None):
            continue
        body, kernel, name = lines[start:i], name, None
        over = [j for j, text in enumerate(body) if re.match(r"^\.Lw_over_wait_\d+:", text)]
        if not over or not demangle(kernel).replace("ocrt::", "").replace("void ", "").startswith("ao_kernel<"):
            continue
        a = max(j for j in range(over[0]) if "ASMSTART" in body[j])
        b = min(j for j in range(over[0], len(body)) if "ASMEND" in body[j])
        report.append(demangle(kernel).replace("ocrt::", "").replace("void ", "") + "   " + " ".join(f"{c:>6s}" for c in CLASSES))
        report.append(class_row("whole kernel", count_classes(body)))
        # the block by labelled stretch
        label, stretch = "entry checks", []
        for text in body[a + 1:b]:
            m = re.match(r"^(\.Lw_[a-z_]+?)_\d+:", text)
            if m:
                if any(instruction_class(t) for t in stretch):
                    report.append(class_row("block: " + label, count_classes(stretch)))
                label, stretch = m.group(1), []
            else:
                stretch.append(text)
        report.append(class_row("block: " + label, count_classes(stretch)))
        # loop depths, as lane_ops_by_place reads them
        depth, depths = 0, []
        for j, text in enumerate(body):
            m = re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)(.*)", text)
            if m:
                note, k = m.group(2), j + 1
                while k < len(body) and re.match(r"^\s+;", body[k]):
                    note += body[k]
                    k += 1
                own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", note)
                inside = re.search(r"in Loop: Header=\S+ Depth=(\d+)", note)
                depth = int(own.group(1)) if own else int(inside.group(1)) if inside else 0
            depths.append(depth)
        walk_depth = depths[a]
        # header of the loop around the block -> ASMSTART
        header = max((j for j in range(a) if re.match(r"^\.LBB\d+_\d+:", body[j]) and depths[j] == walk_depth
                      and re.search(r"Loop Header: Depth=%d" % walk_depth, "".join(body[j:j + 8]))), default=None)
        if header is not None:
            report.append(class_row("loop header -> ASMSTART", count_classes(body[header:a])))
        tail = []
        for text in body[b + 1:]:
            c = instruction_class(text)
            if c in ("VALU", "LDS", "VMEM"):
                break
            tail.append(text)
        report.append(class_row("ASMEND -> first vector instruction", count_classes(tail)))
        outside = [j for j in range(len(body)) if not a <= j <= b]
        for d, what in ((walk_depth, "the turn around the block"), (walk_depth - 1, "per packet"), (walk_depth - 2, "per job")):
            report.append(class_row(f"depth {d}: {what}", count_classes(body[j] for j in outside if depths[j] == d)))
        report.append("")
    return report


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    kernels = parse(open(sys.argv[1]).read())
    if not kernels:
        sys.exit("check_kernel_resources: no kernel-resource-usage remarks found in " + sys.argv[1])
    header = f"{'kernel':44s} {'SGPR':>5s} {'VGPR':>5s} {'scratch':>8s} {'waves/SIMD':>10s} {'SGPR spill':>10s} {'VGPR spill':>10s} {'LDS B':>7s}"
    lines, errors = [header], []
    for k in kernels:
        name = k["name"].replace("ocrt::", "").replace("void ", "")
        row = (f"{name:44s} {k.get('TotalSGPRs', '?'):>5s} {k.get('VGPRs', '?'):>5s} "
               f"{k.get('ScratchSize [bytes/lane]', '?'):>8s} {k.get('Occupancy [waves/SIMD]', '?'):>10s} "
               f"{k.get('SGPRs Spill', '?'):>10s} {k.get('VGPRs Spill', '?'):>10s} {k.get('LDS Size [bytes/block]', '?'):>7s}")
        lines.append(row)
        # hot: the default path = the primary pass's two kernels and the UNIFORM ambient-occlusion pass
        hot = name.startswith(HOT_PRIMARY) or name.startswith("ao_kernel<1, ")
        walker = hot or name.startswith("ao_kernel<")
        if walker and k.get("Occupancy [waves/SIMD]") != "8":
            errors.append(f"{name}: occupancy {k.get('Occupancy [waves/SIMD]')} waves/SIMD, the walk is scheduled for 8")
        if hot and (k.get("VGPRs Spill") != "0" or k.get("ScratchSize [bytes/lane]") != "0"):
            errors.append(f"{name}: VGPR spill {k.get('VGPRs Spill')}, scratch {k.get('ScratchSize [bytes/lane]')} B/lane "
                          "in a hot kernel (walk_collect's fixed registers v56-v62 need the 64-VGPR budget to hold)")
    queries = ("query_kernel<true>", "query_kernel<false>", "query_key_kernel", "query_scatter_kernel", "query_scan_kernel",
               "multihit_walk_kernel<0", "multihit_walk_kernel<1u", "multihit_walk_kernel<2", "multihit_walk_kernel<4",
               "multihit_walk_kernel<8", "multihit_walk_kernel<16", "multihit_resolve_kernel", "ao_query_kernel<1",
               "ao_query_kernel<2", "ao_query_finish_kernel", "layers_kernel<false, false>", "layers_kernel<true, false>", "layers_kernel<true, true>", "views_count_kernel", "views_scan_sums_kernel", "views_order_kernel",
               "views_scatter_kernel", "views_resize_kernel", "ao_mask_kernel<1", "ao_mask_kernel<2", "ao_directional_finish_kernel<1",
               "ao_directional_finish_kernel<2", "ao_rays_kernel<1", "ao_rays_kernel<2",
               "refit_leaves_kernel", "refit_inner_kernel",  # vertex updates (kernels/refit.hip.h): a spill there is memory traffic per record
               # device-side builds (kernels/build.hip.h): a lane per face or node, nothing that should need scratch
               "build_boxes_kernel", "build_root_kernel", "build_keys_kernel", "build_tree_kernel", "build_layout_kernel",
               # device-side instance sets (kernels/instance_build.hip.h): a lane per instance or node, binary64 in registers
               "instance_inverse_kernel", "instance_reach_kernel", "instance_leaves_kernel", "instance_root_kernel",
               "instance_keys_kernel", "instance_tree_kernel", "instance_layout_kernel", "instance_boxes_kernel",
               # closest-point queries (kernels/nearest.hip.h)
               "nearest_key_kernel", "nearest_scatter_kernel", "nearest_coordinates_kernel", "nearest_kernel<false>", "nearest_kernel<true>",
               # segment queries (kernels/segment.hip.h)
               "segment_kernel<true>", "segment_kernel<false>", "visibility_mask_kernel", "visibility_count_kernel",
               "segment_key_kernel", "segment_scatter_kernel",
               # instanced ray queries (kernels/instances.hip.h): two nested exact walks
               "instance_kernel<true>", "instance_kernel<false>",
               # instanced ambient occlusion and views (kernels/instance_views.hip.h): the same nested walks
               "instance_ao_kernel<1", "instance_ao_kernel<2", "instance_layers_kernel",
               # instanced segment queries (kernels/instance_segments.hip.h): the nested walks with the interval at the leaves
               "instance_segment_kernel<true>", "instance_segment_kernel<false>", "instance_visibility_kernel",
               # instanced multi-hit queries (kernels/instance_multihit.hip.h): the nested walks around the lane's list in LDS
               "instance_multihit_walk_kernel<0", "instance_multihit_walk_kernel<1u", "instance_multihit_walk_kernel<2",
               "instance_multihit_walk_kernel<4", "instance_multihit_walk_kernel<8", "instance_multihit_walk_kernel<16",
               "instance_multihit_resolve_kernel",
               # instanced directional occlusion (kernels/instance_directional.hip.h): the nested walks, ao_mask_kernel's tail
               "instance_ao_mask_kernel<1", "instance_ao_mask_kernel<2",
               # signed distance queries (kernels/signed.hip.h): nearest_kernel's walk with a signed tail, and the sign table
               "signed_kernel", "signed_grid_kernel", "sign_keys_kernel", "sign_heads_kernel<", "sign_sum_kernel<", "sign_leaf_kernel")
    # the directional occlusion queries' walk is ao_query_kernel's with another tail (kernels/directional.hip.h): it must keep
    # that kernel's occupancy, 8 waves per SIMD -- a tail that needs more live state than the old one shows here
    full_occupancy = ("ao_mask_kernel<1", "ao_mask_kernel<2")
    # the signed distance queries keep nearest_kernel's register budget: 8 waves per SIMD are what hides its scalar load
    nearest_occupancy = ("nearest_kernel<false>", "signed_kernel", "signed_grid_kernel")
    names = [k["name"].replace("ocrt::", "").replace("void ", "") for k in kernels]
    for p in HOT_PRIMARY:
        if not any(n.startswith(p) for n in names):
            errors.append(f"{p}: not in the remarks (the gate would guard no such kernel: were the kernels renamed?)")
    for q in queries:
        found = [k for k, n in zip(kernels, names) if n.startswith(q)]
        if not found:
            errors.append(f"{q}: not in the remarks (the ray-query kernels must be built)")
        for k in found:
            if k.get("VGPRs Spill") != "0" or k.get("ScratchSize [bytes/lane]") != "0":
                errors.append(f"{q}: VGPR spill {k.get('VGPRs Spill')}, scratch {k.get('ScratchSize [bytes/lane]')} B/lane in a ray-query kernel")
            if k.get("SGPRs Spill") != "0" and q.startswith(("ao_mask_kernel", "ao_directional_finish_kernel", "ao_rays_kernel",
                                                                 "instance_ao_mask_kernel")):
                errors.append(f"{q}: SGPR spill {k.get('SGPRs Spill')} in a directional-occlusion kernel")
            if q in full_occupancy and k.get("Occupancy [waves/SIMD]") != "8":
                errors.append(f"{q}: occupancy {k.get('Occupancy [waves/SIMD]')} waves/SIMD, ao_query_kernel's walk runs at 8")
            if q in nearest_occupancy and k.get("Occupancy [waves/SIMD]") != "8":
                errors.append(f"{q}: occupancy {k.get('Occupancy [waves/SIMD]')} waves/SIMD, the closest-point walk runs at 8")
    if "--isa" in sys.argv:
        places = lane_ops_by_place(open(sys.argv[sys.argv.index("--isa") + 1]).read())
        lines.append("")
        lines.append("SGPR spill traffic (v_readlane / v_writelane) by place: kernel, total, inside the hand-scheduled node loop, "
                     "per turn of the loop around it, per packet, by loop depth")
        for kname, p in places.items():
            short = kname.replace("ocrt::", "").replace("void ", "")
            lines.append(f"{short:44s} {p['total']:5d} {p['in_node_loop']:5d} {p['walk_turn']:5d} {p['per_packet']:5d}   {p['depths']}")
            if not (short.startswith(HOT_PRIMARY) or short.startswith("ao_kernel<1, ")):
                continue
            posed = short.startswith("primary_posed_kernel")
            turn_limit = POSED_LANE_OPS_PER_WALK_TURN if posed else LANE_OPS_PER_WALK_TURN
            packet_limit = POSED_LANE_OPS_PER_PACKET if posed else LANE_OPS_PER_PACKET
            if p["in_node_loop"]:
                errors.append(f"{short}: {p['in_node_loop']} SGPR spill instructions inside the node loop")
            if p["walk_turn"] > turn_limit:
                errors.append(f"{short}: {p['walk_turn']} SGPR spill instructions per turn of the loop around the node loop (limit {turn_limit})")
            if p["per_packet"] > packet_limit:
                errors.append(f"{short}: {p['per_packet']} SGPR spill instructions in the per-packet code (limit {packet_limit})")
        for want in HOT_PRIMARY:
            if not any(k.replace("ocrt::", "").replace("void ", "").startswith(want) for k in places):
                errors.append(f"{want}: no hand-scheduled node loop found in the device assembly")
        lines.append("")
        lines.append("Instructions by class and place, the kernels with the any-hit node loop (static counts; scalar_side_by_place says what the rows are)")
        lines.extend(scalar_side_by_place(open(sys.argv[sys.argv.index("--isa") + 1]).read()))
    table = "\n".join(lines) + "\n"
    if "--table" in sys.argv:
        with open(sys.argv[sys.argv.index("--table") + 1], "w") as f:
            f.write(table)
    print(table, end="")
    if errors and "--report-only" in sys.argv:  # instrumented builds (-DOCRT_STAMPS) carry extra live values
        print("check_kernel_resources (report only): " + "; ".join(errors))
    elif errors:
        sys.exit("check_kernel_resources: " + "; ".join(errors))


if __name__ == "__main__":
    main()
