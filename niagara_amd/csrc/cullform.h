// cullform.h — which kernel a cluster pass launches, decided ONCE, on the host, as a pure function: context.hip fills a CullFormInputs for nv_clustercull and
// nv_taskcull's early pass, choose_cull_form answers with the complete CullForm, launch_cluster_mask (clustercull.hip) dispatches on it without deciding anything
// again.  Plain integer logic, no HIP types: tests/test_cull_form.py builds it with g++ and holds it to a recorded decision table.  Results never depend on it.
#pragma once

#include <stdint.h>

#include "../../include/niagara_vis.h"

namespace nv
{

// CC_DA (template parameter of the cull kernel, clustercull.hip) = ring slots of the filter pass.  The host picks 4 or 8 per launch from the command count of
// the PREVIOUS clustercull (the kernel leaves it in a mapped host word; frame coherence; a wrong guess only costs speed): 4 up to this many commands.
constexpr uint32_t CC_SHALLOW_COMMANDS = 500000;

inline bool clustercull_prefers_shallow(uint32_t previousCommandCount) { return previousCommandCount != 0 && previousCommandCount <= CC_SHALLOW_COMMANDS; }

// the filter pass pays for itself while it finishes more than about half of the commands (measured: DESIGN.md §4.1)
inline bool clustercull_prefers_direct(uint32_t previousCommandCount, uint32_t previousPassedFilter, uint32_t percent)
{
	return previousCommandCount != 0 && (uint64_t)previousPassedFilter * 100u > (uint64_t)previousCommandCount * percent;
}

// The filter form's time goes with the number of COMMANDS (its stream is bound by instruction issue: ~60 instructions per command whatever the command's
// size), the packed direct walk's with the number of valid MESHLETS / 64.  Behind drawcull's LOD select a draw's meshlets end in a partial command — config
// 3B at BASELINE scale: 250 k commands, 40 valid lanes on average — and the packed walk then wins even where the filter rejects nearly everything (22.5 against
// 34 us there, a cache-resident pool; 3A's full commands streamed from HBM: filter 21 us, packed walk 32).  The pass's FILL — valid meshlets per command slot —
// is ESTIMATED, at no cost to any kernel, from what a task pass left for the host anyway (context.hip: emitting draws and commands, hint words 2 and 3): every
// emitting draw ends in one command that is half full on average, fill ~ 1 - draws / (2 commands).  (Round 6 first MEASURED it — the valid meshlets summed by
// the cull kernels, a second word beside the filter statistic, summed by the scatter launch: the scatter launch of the headline pass took 5.09 instead of
// 4.71 us by kernel-trace, whichever part of the plumbing was taken out again; the estimate decides the same way on every config.)
inline bool clustercull_prefers_packed(uint32_t taskCommands, uint32_t emittingDraws, uint32_t fillPercent)
{
	return taskCommands != 0 && emittingDraws != 0 && (uint64_t)(2u * (uint64_t)taskCommands - emittingDraws) * 100u < (uint64_t)taskCommands * 2u * fillPercent;
}

struct CullFormInputs // everything the choice reads
{
	bool taskPayload;                     // nv_taskcull's early pass (the cull launch writes the payloads itself; late is false there), else nv_clustercull
	bool late, soa, filterPositive;       // the pass's late flag; the SoA mirror applies to its meshlet buffer; ClusterArgs::filterK > 0 (the certified test is usable)
	int clusterOcclusionEnabled, postPass; // NvCullData, as given
	int forceDirect, forceShallow;        // NV_OPT_CULL_FORM as stored: value - 1 (-1 = by the statistics); NV_OPT_CULL_RING as stored: -1 / 0 / 1 = by the count / 8 / 4-deep
	uint32_t directPercent;               // share of commands passing the filter above which the launch skips the filter pass
	bool hints;                           // the mapped hint words exist; their values, read once: [0], [1] command count and commands the filter did not (or would not
	uint32_t hint[5];                     // have) finished, of the previous nv_clustercull; [2], [3] emitting draws and commands of the previous task pass of nv_drawcull;
	                                      // [4] command count of the previous nv_taskcull — all possibly a launch or more behind, which only matters for speed
	bool ownTaskCommands;                 // the command list is what this context's last nv_drawcull(task) wrote (good for one launch: the callers clear it)
	uint32_t mirroredCount;               // meshlets of the mirror (is the pool cache-resident?)
	bool alwaysDeep;                      // experiments (debugMode bit 16): never the 4-deep ring by the command count
	uint32_t commandCountOverride;        // ClusterArgs::commandCountOverride
};

struct CullForm // the complete answer
{
	bool lanes;                              // cluster_bits_kernel<soa, true> (one lane per set visibility bit; the rest of the next two lines unset), else
	bool late, soa, bits;                    // cluster_mask_kernel<late, soa, bits, depth, direct, defer, packed>
	int depth;                               // 4 or 8
	bool direct, defer, packed;              // packed: the walk over windows of 64 valid meshlets; it takes the dealing's delay table of its own (dealing.h DEAL_PACKED_TABLE)
	bool twoStage;                           // late pass with HiZ: cluster_hiz_kernel follows the cull launch
	uint32_t deferHiz, packDirect, packBits; // ClusterArgs words of the same names
	uint32_t expectedCmds;                   // the guess of the indirect command count the dealing plan is derived for (0 = none)
	int variant;                             // NV_VARIANT_CULL_*
};

// The statement order is the specification (tests/golden/cull_form_table.npz).
inline CullForm choose_cull_form(const CullFormInputs& in)
{
	const bool task = in.taskPayload;
	// ring depth by the previous command count of the SAME entry point; [0], [1] are a consistent pair of the previous nv_clustercull for either (the payload form
	// writes neither: no scatter launch follows it that would publish its statistic) — a context that only ever calls nv_taskcull stays on the filter form
	const uint32_t previousCmds = task ? in.hint[4] : in.hint[0];
	bool shallow = in.hints && clustercull_prefers_shallow(previousCmds) && !(!task && in.alwaysDeep);
	if (in.forceShallow >= 0)
		shallow = in.forceShallow != 0;
	bool direct = in.hints && clustercull_prefers_direct(in.hint[0], in.hint[1], in.directPercent);
	if (!(in.hints && in.hint[0] != 0) && in.ownTaskCommands) // no statistic yet: by where the commands come from
		direct = true;
	const bool bits = in.clusterOcclusionEnabled == 1 && in.postPass == 0;
	// Late pass with HiZ = three launches: the cull kernel in its early form (frustum + cone ballots), the occlusion probe with one lane per survivor
	// (clustercull.hip cluster_hiz_kernel: visibility bits, skip, tile counts), the scatter.
	const bool twoStage = in.late && in.clusterOcclusionEnabled == 1;
	// A pass of partial commands — what drawcull's LOD select leaves — takes the direct form's packed walk whatever the filter statistic says, where that form
	// exists (early form without visibility bits, over the mirror).  Its fill is estimated from hint words 2 and 3: the emitting draws and commands of the
	// PREVIOUS task pass whose scatter launch has completed — usually not the pass that wrote this list (its launch is still queued on the stream) but the one
	// before, one or more passes behind and possibly another phase's (early / late / post), whose fill differs; a caller's own list is taken as full.
	if (!task && !direct && in.ownTaskCommands && in.hints && in.soa && in.filterPositive && (twoStage || (!in.late && !bits)))
	{
		const bool poolInCache = (uint64_t)in.mirroredCount * 12u <= (48ull << 20);
		direct = clustercull_prefers_packed(in.hint[3], in.hint[2], poolInCache ? 85u : 60u);
	}
	if (in.forceDirect >= 0)
		direct = in.forceDirect != 0;

	CullForm f = {};
	f.soa = in.soa;
	f.twoStage = f.defer = twoStage;
	f.deferHiz = twoStage ? 1u : 0u;
	f.packDirect = !task && in.forceDirect != 3 ? 1u : 0u; // NV_OPT_CULL_FORM 4: one command per wave iteration also where the packed walk applies
	f.packBits = !task && in.forceDirect == 4 ? 1u : 0u;   // NV_OPT_CULL_FORM 5: the early pass with visibility bits as a packed walk too
	// Where the filter would not pay (direct), an EARLY pass with visibility bits tests one LANE per cluster that can be visible at all — per set bit —
	// instead of one wave per command (clustercull.hip cluster_bits_kernel: 26 against 38-40 us at frame scale).  Without bits the direct form walks
	// packed windows of 64 valid meshlets (cluster_mask_kernel PACK, round 6: the cluster pass behind drawcull's LOD select 24 us against 34 for the
	// lane-per-valid-cluster form rounds 4-5 chose for a cache-resident pool, and 44 for one command per wave iteration); so does the late pass's first
	// stage.  NV_OPT_CULL_FORM 3 keeps one wave per command with visibility bits, 4 one command per wave iteration throughout.
	if (!in.late && direct && in.forceDirect < 2 && bits)
	{
		f.lanes = f.bits = true;
		f.variant = NV_VARIANT_CULL_LANES_BITS;
		return f;
	}
	f.late = in.late && !twoStage; // (the two-stage late pass launches the early form)
	f.direct = in.soa && direct && in.filterPositive; // no filter pass: over the mirror only, and the certified test must be usable
	f.depth = !f.direct && !f.late && in.soa && shallow ? 4 : 8; // (the 4-deep ring measured slower for the late pass: 46.7 vs 42.9 us, config 4)
	f.bits = !twoStage && bits;
	// the packed walk exists for the early form without visibility bits (the late pass's first stage is one), over the mirror; with bits on request only
	f.packed = f.direct && !f.late && f.packDirect != 0 && (twoStage || !bits || f.packBits != 0);
	f.expectedCmds = in.commandCountOverride ? in.commandCountOverride : (in.hints ? previousCmds : 0u);
	f.variant = !in.soa ? NV_VARIANT_CULL_AOS : f.direct ? (f.packed ? NV_VARIANT_CULL_DIRECT_PACKED : NV_VARIANT_CULL_DIRECT)
	                                                     : (f.depth == 4 ? NV_VARIANT_CULL_FILTER_RING4 : NV_VARIANT_CULL_FILTER_RING8);
	return f;
}

} // namespace nv
