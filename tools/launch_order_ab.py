#!/usr/bin/env python3
"""In-process, in-frame A/B of the serpentine order per LAUNCH against per DESCRIPTOR on the RRDBNet-23 1080p frame.

The plan's launch list is replayed launch by launch with a HIP event between consecutive launches, as bench.py's kernel classes do, so
every launch runs in the cache state its predecessor leaves.  The two arms use the same build, the same buffers and the same descriptors but
for ``tile_order``; rounds are interleaved.  Classes: the fused pair by shape (conv1+2: 64 input channels, conv3+4: 128), conv5 with one and
with two residuals, everything else.
usage: launch_order_ab.py [rounds [reps]]
"""

import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import resselt_amd  # noqa: E402
from resselt_amd.engine import lib as L  # noqa: E402
from resselt_amd.utils import synth  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device('cuda:0')
model = resselt_amd.load_from_state_dict(dict(synth.rrdbnet_state_dict(nb=23, seed=0))).to(dev)
x = synth.synth_input((1, 3, 1080, 1920), seed=0).to(dev)
keep = model(x)  # fills the plan's buffers; holding the result keeps the last layer's output pointer valid during the replays
torch.cuda.synchronize()
plan = model.last_plan()
stream = torch.cuda.current_stream().cuda_stream
descs = [(arr, i) for arr in plan.conv_arrays for i in range(len(arr))]


def klass(p, fused):
    if fused:
        return f'pair conv{"1+2" if p.cin_planes == 8 else "3+4"} ({p.cin_planes * 8} input channels)'
    if p.cout == 64 and p.cin_planes == 24 and p.res1_hi:
        return 'conv5, two residuals' if p.res2_hi else 'conv5, one residual'
    return 'other convolutions'


def launches():
    """(callable, class) per launch: views into the plan's own arrays, so a re-assigned ``tile_order`` is what the replay runs."""
    out = []
    for arr in plan.conv_arrays:
        i = 0
        while i < len(arr):
            fused = i + 1 < len(arr) and L.conv_pair_fusable(arr[i], arr[i + 1])
            n = 2 if fused else 1
            view = (L.ConvParams * n).from_address(C.addressof(arr[i]))
            out.append((lambda view=view: L.conv2d_list(view, stream), klass(arr[i], fused)))
            i += n
    return out


def assign(arm):
    if arm == 'launch':
        plan.reassign_launch_orders()
    else:
        for k, (arr, i) in enumerate(descs):
            arr[i].tile_order = k & 1


def replay(ls):
    per = {}
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(ls) + 1)]
    evs[0].record()
    for k, (fn, _) in enumerate(ls):
        fn()
        evs[k + 1].record()
    torch.cuda.synchronize()
    for k, (_, name) in enumerate(ls):
        per.setdefault(name, []).append(evs[k].elapsed_time(evs[k + 1]) * 1e3)
    return per, evs[0].elapsed_time(evs[-1])


ls = launches()
names = sorted({name for _, name in ls})
res = {arm: {'frame': [], **{n: [] for n in names}} for arm in ('desc', 'launch')}
for r in range(rounds + 1):  # the first round warms up
    for arm in ('desc', 'launch'):
        assign(arm)
        for _ in range(reps):
            per, frame = replay(ls)
            if r:
                res[arm]['frame'].append(frame)
                for n, us in per.items():
                    res[arm][n].append(statistics.mean(us))
assign('launch')
torch.cuda.synchronize()
L.check_status('launch_order_ab')
count = {n: sum(1 for _, m in ls if m == n) for n in names}
print(f'RRDBNet-23 1080p, convolution launches replayed in frame order, {rounds} interleaved rounds x {reps} passes, aborts={L.ring_aborts()}')
print(f'{"class":44s} {"launches":>8s} {"per descriptor":>16s} {"per launch":>16s} {"change":>8s}')
for n in names:
    a, b = statistics.median(res['desc'][n]), statistics.median(res['launch'][n])
    print(f'{n:44s} {count[n]:8d} {a:13.1f} us {b:13.1f} us {100 * (b - a) / a:+7.2f}%')
a, b = statistics.median(res['desc']['frame']), statistics.median(res['launch']['frame'])
print(f'{"convolution launches of the frame":44s} {len(ls):8d} {a:13.2f} ms {b:13.2f} ms {100 * (b - a) / a:+7.2f}%')
print('frame, every pass (ms): ' + '  '.join(f'{arm}: {" ".join(f"{t:.2f}" for t in res[arm]["frame"])}' for arm in res))
