"""The benchmark script itself: it must run end to end and print ONE JSON line with the contract's fields."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_fields():
    env = dict(os.environ)
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--full', '--steps', '2', '--warmup', '1', '--frames', '2',
                          '--points', '4000', '--no-cpu-baseline'], capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline'):
        assert k in d, k
    assert d['unit'] == 'frames/s' and d['n_gpus'] == 1 and d['steps'] == 2 and d['value'] > 0
    assert 'workload' in d['config'] and 'model' not in d['config']
    r = d['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in r, k
    assert r['bound'] == 'mfma' and 0 < r['frac'] < 1 and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9
    assert d['alt_modes'] and all(a['value'] > 0 for a in d['alt_modes'])
    assert {a['workload'] for a in d['alt_modes']} == {'S1', 'S2'}
    assert 'crop_project' in d['hbm_stages_frac_of_8TBps']
    # the detail file the line names holds everything else
    full = json.load(open(os.path.join(REPO, d['detail'])))
    assert full['config']['frame_sets'] and 'crop_project' in full['hbm_stages'] and full['value'] == d['value']
    assert len(full['alt_modes']) == len(d['alt_modes']) and 'roofline' in full['alt_modes'][0]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_nothing_else(tmp_path):
    """Without --full a run warms up, times its steps and prints the line: the contract's fields and the roofline of its own timed
    steps, but no alternative modes, CPU baseline, second timer pass, host probe, isolated roofline or detail file."""
    detail = tmp_path / 'detail.json'
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '2', '--warmup', '1', '--frames', '2', '--points',
                          '4000'], capture_output=True, text=True, timeout=600, cwd=REPO,
                         env=dict(os.environ, MVX_BENCH_DETAIL=str(detail)))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline'):
        assert k in d, k
    assert d['steps'] == 2 and d['warmup'] == 1 and d['higher_is_better'] is True
    assert abs(d['value'] - 2 * 1e3 / d['ms_per_step']) < 1e-6 * d['value']
    r = d['roofline']
    assert r['bound'] == 'mfma' and 0 < r['frac'] < 1 and r['launches'] > 0 and 'isolated_frac' not in r
    for k in ('alt_modes', 'cpu_baseline', 'other_kernels', 'hbm_stages_frac_of_8TBps', 'host_enqueue_ms_per_step',
              'ms_per_step_all_timers', 'detail'):
        assert k not in d, k
    assert not detail.exists()


@pytest.mark.gpu
def test_default_invocation_prints_a_short_parsable_line_in_the_reference_arithmetic():
    """`python bench.py --full`, every other argument at its default (the r04 line was 27 KB and the driver could not
    parse it).  The line is < 12 KB, one JSON object, with roofline + cpu_baseline; its headline arithmetic is operand-exact (bf16x6 or f32,
    /root/reference/config.yml:2 `half: False`) with fp16x3 as the first alternative, and every alternative mode was timed over >= 20
    steps."""
    env = dict(os.environ)
    env.pop('MVX_CONVMATH', None)
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--full'], capture_output=True, text=True, timeout=1500, env=env,
                         cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    assert len(lines[0]) < 12288, len(lines[0])
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and d['steps'] == 10 and d['warmup'] == 3 and d['value'] > 0
    assert d['dtype'].startswith('f32') and ('bf16x6' in d['dtype'] or d['dtype'] == 'f32') and 'convmath=bf16x6' in d['config']['workload']
    r = d['roofline']
    assert r['bound'] == 'mfma' and 0 < r['frac'] < 1 and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3
    assert d['cpu_baseline']['kind'] == 'port' and d['cpu_baseline']['value'] > 0 and d['cpu_baseline']['cores'] >= 1
    alts = d['alt_modes']
    assert [a['convmath'] for a in alts if a['config'] == 'headline path' and a['workload'] == 'S2'][0] == 'fp16x3'
    assert {a['config'] for a in alts} >= {2, 3, 4}
    assert all(a['steps'] >= 20 and a['value'] > 0 for a in alts)
    assert d['summary'] == d['summary_tail'] and os.path.exists(os.path.join(REPO, d['detail']))


@pytest.mark.gpu
def test_bench_vfe_mode_checks_voxel_indices_against_the_oracle():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--full', '--mode', 'vfe', '--steps', '2', '--warmup', '1',
                          '--frames', '3', '--points', '4000'], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip().startswith('{')][0])
    assert d['roofline']['bound'] == 'hbm' and d['value'] > 0
    assert d['cpu_baseline']['voxel_indices_vs_oracle'].startswith('ok') and d['cpu_baseline']['value'] > 0


@pytest.mark.gpu
def test_bench_full_mode_runs_the_whole_model_and_reports_losses():
    """--mode full (BASELINE config 3): classifyAnchors + frame sets + HIP RPN + VoxelLoss + whole backward inside the step."""
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--full', '--mode', 'full', '--steps', '3', '--warmup', '1',
                          '--frames', '2', '--points', '4000', '--no-cpu-baseline'], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip().startswith('{')][0])
    assert d['config']['mode'] == 'full' and d['value'] > 0 and 'rpn_conv' in d['other_kernels']
    assert len(d['last_losses']) == 2 and all(0 < v < 100 for v in d['last_losses'])


@pytest.mark.gpu
def test_bench_two_ranks_share_the_frames_and_print_one_line():
    """The N > 1 path of bench.py on this one-GPU box: two ranks under torch.distributed.run (gloo instead of RCCL, which
    refuses two ranks on one device), frames {i : i mod 2 = rank}, barrier + MAX over ranks, ONE JSON line from rank 0."""
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MVX_DIST_BACKEND='gloo', MVX_BENCH_FINGERPRINT='1')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                          '127.0.0.1', '--master-port', str(port), os.path.join(REPO, 'bench.py'), '--gpus', '2', '--steps', '2',
                          '--warmup', '1', '--frames', '2', '--points', '4000', '--timed-only'],
                         capture_output=True, text=True, timeout=900, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['scaling'] == 'weak' and d['config']['parallelism'] == 'dp2' and d['value'] > 0
    assert abs(d['value'] - 2 * 2 * d['steps'] / (d['ms_per_step'] * d['steps'] * 1e-3)) < 1e-6 * d['value']
    # the EXCHANGED gradients are right, not only "a number was printed".  Rank 0 ran frames {0, 2}, rank 1 {1, 3};
    # the two-part exchange ([early | late + count] on the communication / training streams) must leave the mean over the four
    # frames in the bucket = the mean of the two ranks' buckets run alone as single processes on the same frames.
    fp2 = d['gradient_fingerprint']
    assert fp2['exchange'].startswith('two-part') and fp2['frame_ids'] == [0, 2]
    singles = []
    for ids in ('0,2', '1,3'):
        o1 = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '1', '--warmup', '0', '--frames', '2', '--points',
                             '4000', '--timed-only', '--frame-ids', ids], capture_output=True, text=True, timeout=600,
                            env=dict(os.environ, MVX_BENCH_FINGERPRINT='1'), cwd=REPO)
        assert o1.returncode == 0, o1.stderr[-2000:]
        singles.append(json.loads([l for l in o1.stdout.splitlines() if l.strip().startswith('{')][0])['gradient_fingerprint'])
    for key in ('sum', 'probe'):
        want = 0.5 * (singles[0][key] + singles[1][key])
        assert abs(fp2[key] - want) <= 1e-5 * max(abs(want), 1e-3 * fp2['norm']), (key, fp2[key], want, fp2['norm'])


@pytest.mark.gpu
def test_bench_fusion_mode_runs_config_4():
    """--mode fusion (BASELINE config 4): FPN feature sampling + fusion MLP + VFE, 2 frames per step, HBM roofline of the sampler."""
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--full', '--mode', 'fusion', '--steps', '2', '--warmup', '1',
                          '--points', '4000', '--no-cpu-baseline'], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip().startswith('{')][0])
    assert d['config']['mode'] == 'fusion' and d['config']['frames_per_gpu'] == 2 and d['value'] > 0
    assert d['roofline']['bound'] == 'hbm' and d['roofline']['launches'] == 2 and 'feature_sample' in d['hbm_stages_frac_of_8TBps']


@pytest.mark.gpu
def test_bench_dumps_what_the_last_timed_step_computed(tmp_path):
    """--dump-outputs DIR: the last timed step's middle maps (a fixed sample), exchanged gradients, parameters after AdamW and
    voxel counts as float .npy files within 64 MiB; --steps is the number of timed steps and ms_per_step their mean time."""
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--timed-only', '--steps', '3', '--warmup', '1', '--frames',
                          '2', '--points', '4000', '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip().startswith('{')][0])
    assert d['steps'] == 3 and d['ms_per_step'] > 0 and abs(d['value'] - 2 * 1e3 / d['ms_per_step']) < 1e-6 * d['value']
    assert sorted(os.listdir(tmp_path)) == ['grad_bucket.npy', 'middle_sample.npy', 'params.npy', 'voxels_per_frame.npy']
    import numpy as np
    a = {n[:-4]: np.load(os.path.join(str(tmp_path), n)) for n in os.listdir(tmp_path)}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert a['voxels_per_frame'].tolist() == [float(v) for v in d['config']['voxels_per_frame']]
    assert a['middle_sample'].shape == (1 << 22,) and np.abs(a['middle_sample']).max() > 0
    assert a['grad_bucket'].shape == a['params'].shape and np.abs(a['grad_bucket']).max() > 0
