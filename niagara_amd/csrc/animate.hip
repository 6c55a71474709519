// animate.hip — nv_animate_draws for gfx950: the keyframe evaluation of src/niagara.cpp:1368-1409 on the device, so that
// moving draws never go through the host: time in, rewritten draw records (and, fused, their cull-mirror entries) out.  The DEFINITION is
// animmath.h, one text with nv_animate_draws_host.
//
// Shape.  One launch, a lane per animation, 256-thread workgroups; nothing is handed between lanes, no LDS, no atomics.  A lane loads its
// record (one 16-byte and one 8-byte load, coalesced across the wave), evaluates the time statements in fp64, gathers its two keyframes
// (4 x 16 bytes), and writes {position, scale} and orientation of its draw as two 16-byte stores; words 8-11 of the draw are never written.
// The validator (host.cpp) guarantees what the kernel relies on: every keyframe index inside the table, every drawIndex below the draw bound
// and every lightIndex below the light bound the entry point checked the buffers against, and no two lanes with the same target.
//
// MIRROR instantiation: the lane reads its draw's meshIndex word and writes the draw's entry of the cull mirror with the text of
// draw_split_kernel (drawmirror.h) from the values it just stored, so that nv_update_draws need not re-read the records.
#include <hip/hip_runtime.h>

#include "animmath.h"
#include "drawmirror.h"
#include "launch.h"

namespace nv
{

constexpr int AN_THREADS = 256;

template <bool MIRROR>
__global__ __launch_bounds__(AN_THREADS) void animate_kernel(const AnimateArgs a)
{
	const uint32_t i = blockIdx.x * (uint32_t)AN_THREADS + threadIdx.x;
	if (i >= a.count)
		return;
	const uint4 rec = a.records[i];
	const float2 tp = a.times[i];
	AnimPhase ph;
	if (!anim_phase(a.time, tp.x, tp.y, rec.w, ph))
		return;
	const float4* k0 = a.keyframes + 2u * ((size_t)rec.z + ph.index0);
	const float4* k1 = a.keyframes + 2u * ((size_t)rec.z + ph.index1);
	const float4 t0 = k0[0], t1 = k1[0]; // translation, scale
	const float t = ph.t;
	const float px = anim_mix(t0.x, t1.x, t), py = anim_mix(t0.y, t1.y, t), pz = anim_mix(t0.z, t1.z, t);
	if ((int32_t)rec.x >= 0 && a.draws)
	{
		const float4 r0 = k0[1], r1 = k1[1];
		const AnimQuat q = anim_slerp(AnimQuat{ r0.x, r0.y, r0.z, r0.w }, AnimQuat{ r1.x, r1.y, r1.z, r1.w }, t);
		const float4 d0 = make_float4(px, py, pz, anim_mix(t0.w, t1.w, t));
		const float4 d1 = make_float4(q.x, q.y, q.z, q.w);
		float4* draw = a.draws + 3u * (size_t)rec.x;
		draw[0] = d0;
		draw[1] = d1;
		if (MIRROR)
		{
			const uint32_t meshIndex = reinterpret_cast<const uint32_t*>(draw + 2)[0];
			const DrawMirrorEntry e = draw_mirror_entry(d0, d1, meshIndex, a.meshes, a.meshCount);
			a.world[rec.x] = e.world;
			a.scaleMesh[rec.x] = e.scaleMesh;
		}
	}
	if ((int32_t)rec.y >= 0 && a.lights)
	{
		float* light = a.lights + 8u * (size_t)rec.y;
		light[0] = px;
		light[1] = py;
		light[2] = pz;
	}
}

int launch_animate(hipStream_t stream, const AnimateArgs& a, bool mirror)
{
	if (a.count)
	{
		const dim3 grid((a.count + AN_THREADS - 1) / AN_THREADS), block(AN_THREADS);
		if (mirror)
			hipLaunchKernelGGL(animate_kernel<true>, grid, block, 0, stream, a);
		else
			hipLaunchKernelGGL(animate_kernel<false>, grid, block, 0, stream, a);
	}
	return (int)hipGetLastError();
}

} // namespace nv
