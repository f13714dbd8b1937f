#!/usr/bin/env python3
"""Pin the tables of the BAM layer (csrc/bamread.cpp through bamio.NativeAlignmentFile): tests/golden/bam_plan.json.

CPU only.  Per case -- a BAM with the index it is read through -- a SHA-256 of everything the plan / scan family hands
out for all of the case's loci: the (n, comp_bytes, out_bytes) of plan() with the chrY regions as `extra`, the four
plan_blocks() arrays, the tasks and chunks of plan_walks / plan_alt_walks / plan_region_walks, the offsets plan_fill()
writes and the payload bytes it copies, the units and every pool of scan(), and those of scan(pe=...) and
scan(pe=..., alt=...) fed with what tests/walk_model.ModelInflater finds over the planned blocks.

  gen_golden_bam_plan.py                 the committed BAMs (t001, t002, synf; t001 and synf also through a CSI-only copy at
                                         min_shift 14) -> tests/golden/bam_plan.json; tests/test_bam_plan.py recomputes it
  gen_golden_bam_plan.py --wide OUT      the file set of tests/test_csi_index.py (synthetic samples, the whole-genome shaped
                                         one, the 300-byte-block file, t001, t002; each with its .bai and with a .csi at 12,
                                         14 and 16), made under OUT/files unless already there -> OUT/<--tag>.json: for
                                         comparing two builds of libtredbam.so over the same files, nothing of it is stored

The tables of the committed BAMs do not depend on the machine's zlib; those of the synthetic files do (their blocks are
deflated when they are made), which is why only the former are committed.
"""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.walk_model import ModelInflater  # noqa: E402
from tredparse_amd import _lib, bamio, synth, synth_bam  # noqa: E402
from tredparse_amd.bam_parser import _site_arrays, y_regions  # noqa: E402
from tredparse_amd.meta import TREDsRepo  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "bam_plan.json")
SHIFTS = (12, 14, 16)


def sha(*arrays):
    """SHA-256 over the arrays' types, shapes and bytes (a bytes object counts as itself)."""
    h = hashlib.sha256()
    for a in arrays:
        if not isinstance(a, bytes):
            a = np.ascontiguousarray(a)
            h.update("{}{};".format(a.dtype.str if a.dtype.names is None else a.dtype.descr, a.shape).encode())
            a = a.tobytes()
        h.update(a)
    return h.hexdigest()


def _scan_hashes(out, key, units, pools):
    out[key + ".units"] = sha(units)
    for k in sorted(pools):
        out["{}.{}".format(key, k)] = sha(pools[k])


def table_hashes(path, repo, names):
    """{table: SHA-256} of one BAM for the loci `names` of `repo` (see the module's text), in a fixed order."""
    f = bamio.NativeAlignmentFile(path)
    try:
        loci = [repo[n] for n in names]
        sites, alts = _site_arrays(repo, names, loci, f)
        ys = y_regions(repo.ref)
        readlen = f.max_read_len(101)
        out = {}
        n, cb, ob = f.plan(sites, alts, readlen, extra=ys)
        out["plan"] = sha(np.array([n, cb, ob], np.int64))
        coffset, clen, crc, host = f.plan_blocks()
        for k, a in (("coffset", coffset), ("clen", clen), ("crc", crc), ("host", host)):
            out["plan_blocks." + k] = sha(a)
        tables = {"walks": f.plan_walks(sites, readlen), "alt_walks": f.plan_alt_walks(sites, alts, readlen),
                  "region_walks": f.plan_region_walks(ys)}
        for k, (tasks, chunks) in tables.items():
            out[k + ".tasks"], out[k + ".chunks"] = sha(tasks), sha(chunks)
        # the device's part, by the model: fill, inflate, walk the regions and the alternative loci
        inf = ModelInflater()
        comp, _, coff, ooff = inf.reserve(cb, ob, n)
        f.plan_fill(inf.comp_addr, 0, 0, coff, ooff)
        out["plan_fill.comp_off"], out["plan_fill.out_off"], out["plan_fill.payload"] = sha(coff), sha(ooff), sha(comp)
        _scan_hashes(out, "scan", *f.scan(sites, alts, readlen))
        tasks, chunks = tables["walks"]
        alt_tasks, alt_chunks = tables["alt_walks"]
        status, dcrc, res, gp, tp, ares, _ = inf.run_walk(n, coffset, clen, crc, tasks, chunks, alt_tasks=alt_tasks,
                                                          alt_chunks=alt_chunks, pool_pairs=_lib.walk_pool_pairs(tasks, ooff))
        inf.run(n)                                       # (every block in the host's copy, as a fetch of all of them leaves it)
        f.preload(inf.out_addr, ooff, status, dcrc)
        _scan_hashes(out, "scan_pe", *f.scan(sites, alts, readlen, pe=(res, gp, tp)))
        _scan_hashes(out, "scan_walked", *f.scan(sites, alts, readlen, pe=(res, gp, tp), alt=ares))
        out["preload.hits_misses"] = sha(np.array(f.preload_clear(), np.int64))
        return out
    finally:
        f.close()


def csi_only(src, dst_dir, min_shift):
    """A copy of the BAM `src` in dst_dir with a .csi of min_shift next to it and no .bai."""
    os.makedirs(dst_dir, exist_ok=True)
    dst = os.path.join(dst_dir, os.path.basename(src))
    shutil.copyfile(src, dst)
    bamio.write_csi(dst, min_shift=min_shift)
    return dst


def committed_cases(tmp):
    """[(case, path, repo, names)] over tests/golden/bam: synf's index is stored gzipped and unpacked next to a copy."""
    repo = TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
    names = sorted(repo.names)
    synf = os.path.join(tmp, "synf.bam")
    shutil.copy(os.path.join(GOLD, "bam", "synf.bam"), synf)
    with gzip.open(os.path.join(GOLD, "bam", "synf.bam.bai.gz"), "rb") as src, open(synf + ".bai", "wb") as dst:
        dst.write(src.read())
    paths = {"t001": os.path.join(GOLD, "bam", "t001.bam"), "t002": os.path.join(GOLD, "bam", "t002.bam"), "synf": synf}
    out = [(k + ".bai", p, repo, names) for k, p in paths.items()]
    out += [(k + ".csi14", csi_only(paths[k], os.path.join(tmp, "csi14"), 14), repo, names) for k in ("t001", "synf")]
    return out


def wide_cases(root):
    """[(case, path, repo, names)] of tests/test_csi_index.py's `files`, made under `root` unless they are there."""
    loci = [l for l in synth.load_loci() if l["name"] in ("HD", "DM1", "SCA1", "AR")]
    manifest = os.path.join(root, "manifest.json")
    if not os.path.exists(manifest):
        os.makedirs(root, exist_ok=True)
        p = synth.SynthParams(coverage=12, expanded_max=120, expanded_frac=0.3)
        made = [(k, path) for k, path, _ in synth_bam.make_bams(root, 2, seed=5, loci=loci, p=p)]
        made += [(k, path) for k, path, _ in synth_bam.make_bams(root, 1, seed=9, prefix="wgs", wgs_like=True)]
        recs, _ = synth_bam.simulate_sample(6, loci[:2], synth.SynthParams(coverage=8, expanded_max=120, expanded_frac=0.3))
        cut = os.path.join(root, "cut300.bam")
        synth_bam.write_bam(cut, recs, sample="cut", block=300, split_records=True, index="both")
        made += [("cut300", cut)] + [(s, os.path.join(GOLD, "bam", s + ".bam")) for s in ("t001", "t002")]
        files = []
        for k, path in made:
            files.append((k + ".bai", path))
            files += [("{}.csi{}".format(k, s), csi_only(path, os.path.join(root, "csi{}".format(s)), s)) for s in SHIFTS]
        with open(manifest, "w") as fp:
            json.dump(files, fp)
    srepo, repo = TREDsRepo(), TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
    out = []
    for case, path in json.load(open(manifest)):
        if case.startswith("t00"):
            out.append((case, path, repo, sorted(repo.names)))
        else:
            names = [l["name"] for l in (synth_bam.bench_loci() if case.startswith("wgs") else loci)]
            out.append((case, path, srepo, names))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--wide", metavar="OUT", help="hash the file set of tests/test_csi_index.py instead, into OUT/<tag>.json")
    ap.add_argument("--tag", default="tables")
    a = ap.parse_args()
    if bamio._native() is None:
        raise SystemExit("tredparse_amd/libtredbam.so is not built")
    with tempfile.TemporaryDirectory() as tmp:
        cases = wide_cases(os.path.join(a.wide, "files")) if a.wide else committed_cases(tmp)
        tables = {case: table_hashes(path, repo, names) for case, path, repo, names in cases}
    out = os.path.join(a.wide, a.tag + ".json") if a.wide else OUT
    doc = {"generator": "tools/gen_golden_bam_plan.py: SHA-256 of the tables bamio.NativeAlignmentFile hands out per BAM and index",
           "tables": tables}
    with open(out, "w") as fp:
        json.dump(doc, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print("wrote {}: {} cases, {} hashes".format(out, len(tables), sum(len(v) for v in tables.values())))


if __name__ == "__main__":
    main()
