// cullform_shim.cpp — host-side window onto niagara_amd/csrc/cullform.h for tests/test_cull_form.py: the SAME header the library's entry points and launchers
// compile, built with g++ at test time.  Test infrastructure.
#include <cstdint>

#include "../niagara_amd/csrc/cullform.h"

extern "C" {

// rows of SHIM_INPUTS words in, rows of SHIM_OUTPUTS words out; the column order is tests/test_cull_form.py's INPUTS / OUTPUTS
enum { SHIM_INPUTS = 19, SHIM_OUTPUTS = 15 };

void shim_choose_cull_form(const uint32_t* in, uint32_t rows, uint32_t* out)
{
	for (uint32_t r = 0; r < rows; ++r, in += SHIM_INPUTS, out += SHIM_OUTPUTS)
	{
		nv::CullFormInputs i = {};
		i.taskPayload = in[0] != 0;
		i.late = in[1] != 0;
		i.clusterOcclusionEnabled = (int)in[2];
		i.postPass = (int)in[3];
		i.soa = in[4] != 0;
		i.filterPositive = in[5] != 0;
		i.forceDirect = (int)in[6] - 1; // as nv_set_option stores NV_OPT_CULL_FORM 0-5: value - 1
		i.forceShallow = in[7] == 0 ? -1 : (in[7] == 4 ? 1 : 0); // as it stores NV_OPT_CULL_RING 0 / 4 / 8
		i.directPercent = in[8];
		i.hints = in[9] != 0;
		for (int k = 0; k < 5; ++k)
			i.hint[k] = in[10 + k];
		i.ownTaskCommands = in[15] != 0;
		i.mirroredCount = in[16];
		i.alwaysDeep = in[17] != 0;
		i.commandCountOverride = in[18];
		const nv::CullForm f = nv::choose_cull_form(i);
		const uint32_t o[SHIM_OUTPUTS] = {f.lanes,            f.late,     f.soa,        f.bits,     (uint32_t)f.depth, f.direct,      f.defer,         f.packed,
		                                  f.twoStage,         f.deferHiz, f.packDirect, f.packBits, f.expectedCmds,    f.packed, (uint32_t)f.variant};
		for (int k = 0; k < SHIM_OUTPUTS; ++k)
			out[k] = o[k];
	}
}
}
