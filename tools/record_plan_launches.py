"""Record what the perceptual plan launches and computes: tests/golden/plan_launches.json.

The host engine (csrc/plan.hip) decides, per conv slot and direction, which kernel runs.  A change to how it decides
must leave two things alone: the ordered list of launch brackets of every call (``PerceptualPlan.profile_launches()``:
family and VGG module) and the bytes of every result.  This tool records both for a set of small cases; run it on the
commit whose behaviour is to be kept, commit the file, and tests/test_gpu_plan_routes.py replays the same cases
(``CASES`` / ``run_case`` below are the one definition both use) against it.

Every case runs twice here and the hashes must agree (the kernels on this path hold no floating-point atomics); the
tool exits non-zero where they do not, after writing the file with those cases' hashes left out and their names listed
under "nondeterministic".

The test replays ``CASES``, ``_inputs`` and ``_calls`` as they stand in this file: changing any of them changes what the
recorded hashes mean, so it requires recording again, on the commit the fixture names.

    python tools/record_plan_launches.py [--out tests/golden/plan_launches.json] [--commit HASH]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "2d-to-3d-style-transfer_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# every switch that decides a route; a case sets its own and clears the rest
SWITCHES = ("ST3D_CONV", "ST3D_WINO43", "ST3D_WINO43_MINK", "ST3D_PREGATE", "ST3D_TAP0_FUSED", "ST3D_NEED_DEPTH",
            "ST3D_FLAT_DEPTH", "ST3D_FLAT", "ST3D_GRAPH", "ST3D_W43_SLOTS")

_ENVS_FULL = ([{}, {"ST3D_WINO43": "0"}, {"ST3D_WINO43_MINK": "128"}, {"ST3D_CONV": "direct"}, {"ST3D_PREGATE": "0"},
               {"ST3D_TAP0_FUSED": "0"}, {"ST3D_WINO43": "0", "ST3D_PREGATE": "0", "ST3D_TAP0_FUSED": "0"}] +
              [{"ST3D_NEED_DEPTH": str(k)} for k in range(3)] + [{"ST3D_FLAT_DEPTH": str(k)} for k in range(3)] +
              [{"ST3D_FLAT": "0"}])
_ENVS_SMALL = [{}, {"ST3D_CONV": "direct"}]


def case_name(B, S, env):
    return "B%d_S%d" % (B, S) + "".join("_%s=%s" % (k[5:], env[k]) for k in sorted(env))


# (B, S, env): S = 64 is the smallest size with every route (F(4x4,3x3) at conv1_2 .. conv2_2, F(2x2,3x3) above, the fused
# relu1_1 pass, 3 need levels, 3 flat levels), 128 the same one level deeper; 48: no F(4x4,3x3), no lists, direct kernels
# from 6x6 down; 50: W % 4 != 0 and odd pooled sizes, direct kernels throughout; 16: the smallest size a plan accepts
CASES = ([(2, 64, e) for e in _ENVS_FULL] + [(1, 128, e) for e in _ENVS_FULL] +
         [(B, S, e) for B, S in ((2, 48), (1, 50), (1, 16)) for e in _ENVS_SMALL])

COLOR = (0.125, 0.5, 0.625)
# backward of forward(upto=30): a tap on a ReLU module (6), on a conv whose output feeds a pool while a pooled gradient
# arrives (7: the unpool-and-add pass), on a pool module (18) and on the top module (30)
BACKWARD_UPTO, BACKWARD_TAPS = 30, (6, 7, 18, 30)


def _rect(S):
    return 3 * S // 8, 5 * S // 8, S // 4, 3 * S // 4          # y0, y1, x0, x1: centred


def _inputs(n, S, dev):
    """seeded: content, one style image, n style images, a full-noise image, and the image of the mask / colour calls --
    the colour everywhere but a centred rectangle of noise, with that rectangle as its need mask"""
    import torch
    g = torch.Generator().manual_seed(1000 * S + n)
    content, style_n, cur = (torch.rand((n, 3, S, S), generator=g) for _ in range(3))
    style_1 = torch.rand((1, 3, S, S), generator=g)
    y0, y1, x0, x1 = _rect(S)
    flat = torch.tensor(COLOR).view(1, 3, 1, 1).expand(n, 3, S, S).clone()
    flat[:, :, y0:y1, x0:x1] = torch.rand((n, 3, y1 - y0, x1 - x0), generator=g)
    mask = torch.zeros((n, S, S), dtype=torch.uint8)
    mask[:, y0:y1, x0:x1] = 1
    return [t.to(dev) for t in (content, style_1, style_n, cur, flat, mask)], g


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _calls(plan, n, S, dev):
    """the calls of one case with n images, as (name, thunk -> tensors to hash)"""
    import torch
    (content, style_1, style_n, cur, flat, mask), g = _inputs(n, S, dev)
    sw, cw = 1e6, 1.0

    def loss(img, **kw):
        l, gr = plan.loss(img, sw, cw, **kw)
        return (l,) if gr is None else (l, gr)

    def set_content():
        plan.set_content(content, force=True)
        return ()

    def set_style(style):
        plan.set_style(style, n, force=True)
        return ()

    def graph_on():
        plan.use_graph(True)
        return loss(cur)

    def graph_off():
        out = loss(cur)
        plan.use_graph(False)
        return out

    def forward(upto):
        plan.forward(cur, upto=upto)
        return (plan.activation(upto, n),)

    def backward():
        plan.forward(cur, upto=BACKWARD_UPTO)
        grads = {m: torch.randn(tuple(plan.activation(m, n).shape), generator=g).to(dev) for m in BACKWARD_TAPS}
        return (plan.backward(grads, BACKWARD_UPTO),)

    # pool5 of a 16x16 image would pool a 1x1 map: the deepest module such a plan can run is relu5_4
    top = 36 if S >= 32 else 35
    return [("set_content", set_content), ("set_style_1", lambda: set_style(style_1)), ("set_style_n", lambda: set_style(style_n)),
            ("loss_nograd", lambda: loss(cur, want_grad=False)), ("loss", lambda: loss(cur)),
            ("loss_need", lambda: loss(flat, need_mask=mask)), ("loss_flat", lambda: loss(flat, flat_color=COLOR)),
            ("loss_need_flat", lambda: loss(flat, need_mask=mask, flat_color=COLOR)),
            ("graph_plain", graph_on), ("graph_capture", lambda: loss(cur)), ("graph_replay", graph_off),
            ("forward_%d" % top, lambda: forward(top)), ("backward_%d" % BACKWARD_UPTO, backward)]


def run_case(B, S, dev=None):
    """-> {"<call>@n<k>": {"launches": [[family, module], ...], "sha256": hex or None (nothing to hash)}} for a fresh handle
    and plan under the environment as it is now (the handle reads its switches when it is made).  A plan of B = 2 runs the
    calls with 2 images and then with 1.  Hashes come from a pass with profiling off (profiling bypasses graph replay),
    launch lists from a second, profiled pass of the same calls."""
    import torch
    from st3d import vgg as V
    dev = dev or torch.device("cuda:0")
    net = V.Vgg19Features(_state(), device=dev)
    plan = V.PerceptualPlan(net, B, S)
    out = {}
    try:
        for prof in (False, True):
            plan.profile(prof)
            for n in sorted({B, 1}, reverse=True):
                for name, thunk in _calls(plan, n, S, dev):
                    res = thunk()
                    torch.cuda.synchronize()
                    rec = out.setdefault("%s@n%d" % (name, n), {})
                    if prof:
                        rec["launches"] = [[f, m] for f, m, _ in plan.profile_launches()]
                    else:
                        rec["sha256"] = _sha(*res) if res else None
        plan.profile(False)
    finally:
        plan.close()
    return out


_STATE = []


def _state():
    from st3d import vgg as V
    if not _STATE:
        _STATE.append(V.synthetic_state(0))
    return _STATE[0]


def dump(doc):
    """the fixture's text: one launch list and one case per line, so that a diff of the file can be read"""
    js = lambda o: json.dumps(o, separators=(",", ":"))
    head = ",\n".join('"%s":%s' % (k, js(doc[k])) for k in ("recorded_at_commit", "recorder", "nondeterministic"))
    lists = ",\n".join(js(l) for l in doc["launch_lists"])
    cases = ",\n".join("%s:%s" % (js(k), js(v)) for k, v in doc["cases"].items())
    return '{%s,\n"launch_lists":[\n%s\n],\n"cases":{\n%s\n}}\n' % (head, lists, cases)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "plan_launches.json"))
    ap.add_argument("--commit", default=None, help="hash of the commit being recorded (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    cases, unstable = {}, []
    for B, S, env in CASES:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        name = case_name(B, S, env)
        first, second = run_case(B, S), run_case(B, S)
        bad = sorted(c for c in first if first[c] != second[c])
        if bad:
            unstable.append(name)
            print("NOT REPRODUCED: %s: %s" % (name, ", ".join(bad)), flush=True)
            for c in first.values():
                c["sha256"] = None
        fams = {f for c in first.values() for f, _ in c["launches"]}
        if not env and S in (64, 128):     # a fixture that only ever saw full launches would check nothing
            want = {"conv43_dgrad_need", "convx_dgrad_need", "conv43_fwd_flat", "flat_fill"}
            assert want <= fams, (name, sorted(want - fams))
            assert not bad, "the default environment does not reproduce its own bits: " + name
        cases[name] = {"B": B, "S": S, "env": env, "calls": first}
        print("%-60s %3d calls, %4d launches" % (name, len(first), sum(len(c["launches"]) for c in first.values())), flush=True)
    for k in SWITCHES:
        os.environ.pop(k, None)
    lists = []          # most calls share a launch list with others: each distinct list is stored once, calls hold its index
    for case in cases.values():
        for c in case["calls"].values():
            if c["launches"] not in lists:
                lists.append(c["launches"])
            c["launches"] = lists.index(c["launches"])
    doc = {"recorded_at_commit": commit, "recorder": "tools/record_plan_launches.py", "nondeterministic": unstable,
           "launch_lists": lists, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(dump(doc))
    print("wrote %s (%d cases, %d bytes)" % (a.out, len(cases), os.path.getsize(a.out)))
    return 1 if unstable else 0


if __name__ == "__main__":
    sys.exit(main())
