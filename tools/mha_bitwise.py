"""Bit-for-bit record of the attention kernels: sha256 of every output of the five raw entry points of
mha.hip on seeded inputs, one JSON per library, and a comparison of two such records.

  python tools/mha_bitwise.py > branch.json
  RSX_LIB_PATH=/path/to/parent/librecsys_amd.so python tools/mha_bitwise.py > parent.json
  python tools/mha_bitwise.py --compare parent.json branch.json   # writes profiles/mha_unify_bitwise.json

One process per library (RSX_LIB_PATH picks it). Every output buffer is pre-filled with one finite value,
so a missing or a stray write changes a hash. Cases: each (precision, head dim) row of the table in
tests/test_gpu_dropout_exact.py; 7 sequences, dense at L in {1, 16, 17, 33, 48, 64} (1 .. 4 16-token
blocks) and packed with lengths {1, 16, 17, 33, 48, 64, 0} (head dim 64 also packed with lengths <= 32 at
L = 32: mha_bwd64_k<32>); causal or not; key pad present (dense: left padding, packed: the last key) or
absent; p in {0, 0.2} with a seed whose high word is set.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -7.25
SEED = (0x9E3779B9 << 32) | 0x1234567
B = 7
DENSE_L = (1, 16, 17, 33, 48, 64)
PACKED = {"packed64": ((1, 16, 17, 33, 48, 64, 0), 64)}
PACKED_DH64 = {"packed32": ((1, 16, 17, 32, 5, 31, 0), 32)}
# row name: (forward entry, backward entry, head dim, heads)
ROWS = {
    "fp32_dh16": ("rsx_mha_fwd", "rsx_mha_bwd", 16, 2),
    "fp32_dh32": ("rsx_mha_fwd", "rsx_mha_bwd", 32, 2),
    "fp32_dh64": ("rsx_mha_fwd", "rsx_mha_bwd", 64, 1),
    "bf16x3_dh32": ("rsx_mha_fwd_x3", "rsx_mha_bwd_x3", 32, 2),
    "bf16x3_dh64": ("rsx_mha_fwd_x3", "rsx_mha_bwd", 64, 1),
    "fused_dh32": ("rsx_mha_qkv_fwd_x3", "rsx_mha_bwd_x3", 32, 4),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def layouts(dh):
    """name -> (lengths or None for dense, L)"""
    out = {f"dense{L}": (None, L) for L in DENSE_L}
    out.update(PACKED)
    if dh == 64:
        out.update(PACKED_DH64)
    return out


def record():
    import torch

    sys.path.insert(0, ROOT)
    import recsys_amd  # noqa: F401
    from recsys_amd import _native as N

    dev = torch.device("cuda", 0)
    lib = N.lib()
    res = {}
    for row, (fwd, bwd, dh, H) in ROWS.items():
        D = H * dh
        for lay, (lens, L) in layouts(dh).items():
            g = torch.Generator(device="cpu").manual_seed(1000 + 64 * dh + L + (0 if lens is None else 7))
            if lens is None:
                T, seg = B * L, None
                pad = torch.zeros(B, L, dtype=torch.uint8)
                for b in range(B):
                    pad[b, :min(b % 4, L - 1)] = 1  # left padding, at least one key left
                pad = pad.reshape(-1)
            else:
                T = sum(lens)
                off = [0]
                for n in lens:
                    off.append(off[-1] + n)
                seg = torch.tensor(off, dtype=torch.int32, device=dev)
                pad = torch.zeros(T, dtype=torch.uint8)
                for b, n in enumerate(lens):
                    if n > 1:
                        pad[off[b + 1] - 1] = 1  # the sequence's last key
            qkv_in = torch.randn(T, 3 * D, generator=g).to(dev)
            x = torch.randn(T, D, generator=g).to(dev)
            w = (torch.randn(3 * D, D, generator=g) / D ** 0.5).to(dev)
            bias = torch.randn(3 * D, generator=g).to(dev)
            dout = torch.randn(T, D, generator=g).to(dev)
            pad = pad.to(dev)
            for causal in (1, 0):
                for kp in (pad, None):
                    for p in (0.0, 0.2):
                        name = f"{row}/{lay}/{'causal' if causal else 'full'}/{'pad' if kp is not None else 'nopad'}/p{p}"
                        out = torch.full((T, D), FILL, device=dev)
                        lse = torch.full((T, H), FILL, device=dev)
                        dqkv = torch.full((T, 3 * D), FILL, device=dev)
                        if fwd == "rsx_mha_qkv_fwd_x3":
                            qkv = torch.full((T, 3 * D), FILL, device=dev)
                            rc = lib.rsx_mha_qkv_fwd_x3(N.ptr(x), N.ptr(w), N.ptr(bias), N.ptr(kp), N.ptr(seg), B, L, H,
                                                        causal, p, SEED, N.ptr(qkv), N.ptr(out), N.ptr(lse), N.stream())
                            N.check(rc, fwd)
                            res[f"{name}/qkv"] = sha(qkv)
                        else:
                            qkv = qkv_in
                            rc = getattr(lib, fwd)(N.ptr(qkv), N.ptr(kp), N.ptr(seg), B, L, H, dh, causal, p, SEED,
                                                   N.ptr(out), N.ptr(lse), N.stream())
                            N.check(rc, fwd)
                        rc = getattr(lib, bwd)(N.ptr(qkv), N.ptr(kp), N.ptr(seg), N.ptr(out), N.ptr(lse), N.ptr(dout), B, L,
                                               H, dh, causal, p, SEED, N.ptr(dqkv), N.stream())
                        N.check(rc, bwd)
                        torch.cuda.synchronize()
                        res[f"{name}/out"] = sha(out)
                        res[f"{name}/lse"] = sha(lse)
                        res[f"{name}/dqkv"] = sha(dqkv)
    print(json.dumps({"library": os.path.realpath(N.LIB_PATH), "build_hash": lib.rsx_build_hash().decode(),
                      "outputs": res}, sort_keys=True), flush=True)


def compare(pa, pb):
    a, b = (json.load(open(p)) for p in (pa, pb))
    oa, ob = a["outputs"], b["outputs"]
    names = sorted(set(oa) | set(ob))
    eq = {n: oa.get(n) is not None and oa.get(n) == ob.get(n) for n in names}
    fam = {}
    for n in names:
        f = fam.setdefault(n.split("/")[0], {"compared": 0, "equal": 0})
        f["compared"] += 1
        f["equal"] += int(eq[n])
    rep = {
        "what": "sha256 of every output of the parent's library and this tree's on the same seeded inputs, one process "
                "per library (tools/mha_bitwise.py)",
        "parent_library": "librecsys_amd.so built from the parent commit, source hash " + a["build_hash"],
        "branch_library": "librecsys_amd.so built from this tree, source hash " + b["build_hash"],
        "all_equal": all(eq.values()),
        "by_family": fam,
        "not_equal": [n for n in names if not eq[n]],
        "outputs": eq,
    }
    path = os.path.join(ROOT, "profiles", "mha_unify_bitwise.json")
    with open(path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"all_equal": rep["all_equal"], "compared": len(names), "not_equal": len(rep["not_equal"])}))
    return 0 if rep["all_equal"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_JSON", "BRANCH_JSON"))
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else record())
