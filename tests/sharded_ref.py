"""A sharded frame on the CPU (test infrastructure): one OracleRank per draw range runs the oracle's passes and the reference raster
(tests/raster_ref.py) on d_draws + begin exactly as pipeline.ShardedVisibilityPipeline runs the HIP passes, and `stitched` puts the ranks'
records back together with niagara_amd.shard's helpers in the layout of raster_ref.oracle_frames' records."""
import numpy as np

import oracle
import raster_ref as RR
from niagara_amd import layouts as L
from niagara_amd import shard

PHASES = {"early": (0, 0), "late": (1, 0), "post": (1, 1)}


def phase_names(post_pass):
    return ["early", "late"] + (["post"] if post_pass else [])


class OracleRank:
    def __init__(self, scene, begin, end, rref):
        self.scene, self.begin, self.end, self.rref = scene, begin, end, rref
        self.draws = scene["draws"].copy()
        slots, _ = oracle.assign_visibility_offsets(self.draws, scene["meshes"])  # the GLOBAL prefix
        self.local = self.draws[begin:end]
        self.dvb = np.zeros(max(1, end - begin), np.uint32)
        self.mvb = np.zeros(max(1, (slots + 31) // 32 + 2), np.uint32)
        w, h = scene["viewport"]
        self.pyr = oracle.Pyramid(w, h)
        self.depth = np.zeros((h, w), np.float32)

    def phase(self, name):
        """one phase up to and including its raster (self.depth: the rank's own draws on top of what it loaded); returns the record"""
        s, (late, pp) = self.scene, PHASES[name]
        w, h = s["viewport"]
        if name == "late":
            oracle.depthreduce(self.depth, self.pyr)
        cd = s["cull"].copy()
        cd["drawCount"] = self.end - self.begin
        pd = cd.copy()
        pd["clusterBackfaceEnabled"] = 1 if pp == 0 else 0
        pd["postPass"] = pp
        co, c4 = np.zeros(4096 + 64, dtype=L.TASKCMD), np.zeros(4, np.uint32)
        oracle.drawcull(pd, late, 1, self.local, s["meshes"], co, c4, self.dvb, self.pyr)
        oracle.tasksubmit(c4, co)
        ncmd = int(c4[1]) * 64
        cc = cd.copy()
        cc["postPass"] = pp
        cib, cc4 = np.zeros(ncmd * 64 + 256, np.uint32), np.zeros(4, np.uint32)
        oracle.clustercull(cc, late, co, c4, self.local, s["meshlets"], self.mvb, self.pyr, cib, cc4)
        oracle.clustersubmit(cc4, cib)
        g = RR.globals_for(cd, (w, h), pp)
        self.depth, _, tot = self.rref.raster(g, co, self.local, s["meshlets"], s["data"], s["vertices"], cib, cc4, w, h,
                                              depth=None if name == "early" else self.depth)
        return dict(count4=c4.copy(), commands=co[:int(c4[0])].copy(), cc4=cc4.copy(), cib=cib[:int(cc4[0])].copy(), dvb=self.dvb[:self.end - self.begin].copy(),
                    mvb=self.mvb.copy(), samples=int(tot[3]))


def stitched(per_rank, ranges):
    """per_rank[r]: a phase record of rank r (commands / cib WITHOUT submit padding, dvb over its own draws, full-size mvb) -> the phase
    record of the unsharded frame: count4 / cc4 rebuilt and the lists padded by the oracle's submit passes"""
    commands = shard.stitch_commands([p["commands"] for p in per_rank], ranges)
    ids = shard.stitch_cluster_ids([p["cib"] for p in per_rank], [len(p["commands"]) for p in per_rank])
    dvb, mvb = shard.stitch_visibility([p["dvb"] for p in per_rank], [p["mvb"] for p in per_rank])
    out = dict(dvb=dvb, mvb=mvb, n_commands=len(commands), n_clusters=len(ids), commands_unpadded=commands)
    if commands.dtype == L.TASKCMD:
        co, c4 = np.zeros(len(commands) + 64, dtype=L.TASKCMD), np.zeros(4, np.uint32)
        co[:len(commands)], c4[0] = commands, len(commands)
        oracle.tasksubmit(c4, co)
        cib, cc4 = np.concatenate([ids, np.zeros(512, np.uint32)]), np.zeros(4, np.uint32)
        cc4[0] = len(ids)
        oracle.clustersubmit(cc4, cib)
        out.update(count4=c4, commands=co[:int(c4[1]) * 64], cc4=cc4, cib=cib[:int(cc4[2]) * 256])
    return out


def lockstep_frames(scene, ranges, frames, post_pass, rref, composite=True):
    """every rank of `ranges` stepped phase by phase in this process, the composite as np.maximum on the bit patterns (composite=False:
    the negative control, every rank keeps its own depth).  One record per frame: per phase the stitched record + "depth" (the maximum over
    the ranks) + "samples" per rank; "pyramid" per rank"""
    ranks = [OracleRank(scene, b, e, rref) for b, e in ranges]
    out = []
    for _ in range(frames):
        rec = {}
        for name in phase_names(post_pass):
            parts = [r.phase(name) for r in ranks]
            full = ranks[0].depth.view(np.uint32).copy()
            for r in ranks[1:]:
                full = np.maximum(full, r.depth.view(np.uint32))
            if composite:
                for r in ranks:
                    r.depth = full.view(np.float32).copy()
            rec[name] = dict(stitched(parts, ranges), depth=full.view(np.float32).copy(), samples=[p["samples"] for p in parts])
        rec["pyramids"] = [r.pyr.data.copy() for r in ranks]
        out.append(rec)
    return out


def same_phase(got, want):
    """the stitched phase record equals the unsharded oracle's (raster_ref.oracle_frames)"""
    for k in ("count4", "commands", "cc4", "cib", "dvb", "mvb"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["depth"].view(np.uint32).tobytes() == want["depth"].view(np.uint32).tobytes(), "depth"


def assert_not_vacuous(scene, ranges, unsharded, early_samples):
    """the issue's conditions on a scene / split: non-empty ranges; at least two ranks rasterise something in an early phase; the late pass
    of frame 2 rejects draws that frame 1's late pass (empty pyramid) kept, and one of them belongs to another rank than the occluder."""
    assert all(e > b for b, e in ranges)
    rank_of = lambda d: next(r for r, (b, e) in enumerate(ranges) if b <= d < e)
    kept_empty, kept = unsharded[0]["late"]["dvb"], unsharded[1]["late"]["dvb"]
    rejected = [d for d in range(len(scene["draws"])) if kept_empty[d] == 1 and kept[d] == 0]
    assert rejected, "the late pass rejects nothing"
    occluders = scene.get("wall") or scene.get("surfaces")
    if len(ranges) > 1:
        assert early_samples is None or sum(1 for s in early_samples if s > 0) >= 2, early_samples
        assert any(rank_of(d) not in {rank_of(o) for o in occluders} for d in rejected), "every rejected draw sits on its occluder's rank"
    return rejected
