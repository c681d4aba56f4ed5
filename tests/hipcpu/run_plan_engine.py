"""TEST INFRASTRUCTURE -- run the planner-tail kernels of csrc/stp3_plan.hip (stp3_plan_scene, stp3_plan_drive) on CPU tensors
through libstp3hip_cpu.so (tests/hipcpu/build.py) on the cases of tests/plan_engine_cases.py and store what they wrote.

    python tests/hipcpu/run_plan_engine.py <libstp3hip_cpu.so> <out.npz>

Driver of tests/test_plan_engine_cpu.py (which holds the checks).  ``reduce_channel`` runs in plain torch BEFORE the binding is
pointed at the host library.  Per case ``<name>/``: final, selected, index (+ occupancy, lane, drivable of the scene kernel):
  golden        the inputs of tests/golden/planning.npz (planner/eval/traj)
  target, zero  the two cases of tests/golden/plan_engine.npz
  scene_f32, scene_bf16, scene_cl   the scene kernel on random logits (float32, bf16, permuted strides)
  select, tie   N = 1 800, T = 6, B = 4; ``tie``: in every sample a neighbour of the winner overwritten with the winner's row"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'st-p3_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(lib_path, out_path):
    from run_sampler import setup
    from stp3_amd.config import perception_cfg
    from stp3_amd.models.planning_model import Planning
    from tests import plan_engine_cases as PC
    from tests.test_planning_cpu import PLANNING
    cfg = perception_cfg(**PLANNING)
    big = perception_cfg(**{**PLANNING, 'N_FUTURE_FRAMES': 6, 'PLANNING.SAMPLE_NUM': 1800})
    jobs = []                                              # (name, planner, h0, scene inputs, trajs, cost volume, commands, target)
    with torch.no_grad():
        pl, ins = PC.golden_planner(cfg)
        h0 = pl.reduce_channel(ins['cam_front']).flatten(start_dim=1).float()
        jobs.append(('golden', pl, h0, (PC.logits_of(ins['occupancy']), None, ins['hdmap_logits'], 0), ins['sample_trajs'],
                     ins['cost_volume'], ins['commands'], ins['target']))
        pl = PC.planner(cfg, Planning)
        for name, zero in (('target', False), ('zero', True)):
            ins = PC.inputs(cfg, zero_target=zero)
            h0 = pl.reduce_channel(ins['cam_front']).flatten(start_dim=1).float()
            jobs.append((name, pl, h0, (ins['segmentation'], ins['pedestrian'], ins['hdmap'], ins['n_present']), ins['trajs'],
                         ins['cost_volume'], ins['commands'], ins['target']))
        plb = PC.planner(big, Planning)
        ins = PC.selection_case(big)
        h0 = plb.reduce_channel(ins['cam_front']).flatten(start_dim=1).float()
        jobs.append(('select', plb, h0, (ins['segmentation'], ins['pedestrian'], ins['hdmap'], ins['n_present']), ins['trajs'],
                     ins['cost_volume'], ins['commands'], ins['target']))
    setup(lib_path)
    from stp3_amd import ops_plan
    out = {}
    for name, planner, h0, scene, trajs, cv, commands, target in jobs:
        occupancy, lane, drivable = ops_plan.plan_scene(*scene)
        codes = ops_plan.command_codes(commands)
        final, selected, index = ops_plan.plan_drive(planner, trajs, cv, occupancy, lane, drivable, codes, target, h0)
        again = ops_plan.plan_drive(planner, trajs, cv, occupancy, lane, drivable, codes, target, h0)
        assert all(torch.equal(a, b) for a, b in zip(again, (final, selected, index)))
        for k, v in (('final', final), ('selected', selected), ('index', index), ('occupancy', occupancy), ('lane', lane),
                     ('drivable', drivable)):
            out[f'{name}/{k}'] = v.numpy()
        if name == 'select':
            tied = trajs.clone()
            other = []
            for b, command in enumerate(commands):
                lo, hi = PC.command_range(command, trajs.shape[1])
                win = int(index[b])
                j = win - 1 if win > lo else win + 1
                tied[b, j] = trajs[b, win]
                other.append(j)
            f2, s2, i2 = ops_plan.plan_drive(planner, tied, cv, occupancy, lane, drivable, codes, target, h0)
            out['tie/final'], out['tie/selected'], out['tie/index'], out['tie/other'] = f2.numpy(), s2.numpy(), i2.numpy(), np.array(other)
    for name, dtype, permute in (('scene_f32', torch.float32, False), ('scene_bf16', torch.bfloat16, False), ('scene_cl', torch.float32, True)):
        seg, ped, hd, n_present, _ = PC.scene_case(dtype)
        if permute:                                        # channels-last memory under the same logical shape
            seg = seg.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
            ped = ped.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
            hd = hd.contiguous(memory_format=torch.channels_last)
            assert not seg.is_contiguous() and not hd.is_contiguous()
        for k, v in zip(('occupancy', 'lane', 'drivable'), ops_plan.plan_scene(seg, ped, hd, n_present)):
            out[f'{name}/{k}'] = v.numpy()
    occ_only = ops_plan.plan_scene(*PC.scene_case()[:1], None, *PC.scene_case()[2:4])
    out['scene_noped/occupancy'] = occ_only[0].numpy()
    np.savez(out_path, **out)
    print('RESULT', out_path)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
