"""Stage sequencing (reference src/decombinator/pipeline.py:10-58).  This build implements stage 1 (`decombine`, on the
GPU) and the per-row front half of stage 2 (`collapse`: spacer search, UMI extraction, barcode quality and length filters —
collapse.read_in_data up to where it starts grouping rows, collapse.py:482-565).  The grouping / clustering rest of
`collapse` and the `translate` stage are host stages of the reference that BASELINE.json's north_star leaves on the host
(`translate.get_cdr3` is available as a function: decombinator_amd/translate.py).  `pipeline` therefore writes the `.n12`,
runs the front half over the rows and reports its counters.  With `cluster` (--cluster) it is the reference's run
(pipeline.py:10-38): decombine, the whole of `collapse` (collapse.collapsinator: grouping, UMI clustering on the GPU,
counting), then `translate`, writing the `.n12`, `.freq` and `.tsv`."""
from __future__ import annotations

from datetime import datetime
from typing import Any, Optional

from . import collapse
from . import decombine as dec
from .decombine import decombinator
from .io import cli_args, write_out_counts, write_out_intermediate


def clonotype_refusal(inp: dict):
    """Why --clonotypes cannot run with these arguments, or None: it needs a stage that counts DCRs in front of translate."""
    if not inp.get("clonotypes"):
        return None
    if inp["command"] in ("decombine", "collapse"):
        return (f"--clonotypes belongs to the translate step: {inp['command']} does not translate (translate --clonotypes, or "
                "pipeline --cluster / -nbc --count-dcrs with --clonotypes)")
    if inp["command"] == "pipeline" and not (inp.get("cluster") or inp.get("count_dcrs")):
        return "--clonotypes needs counted DCRs: run pipeline with --cluster (barcoded) or -nbc --count-dcrs (barcode-free)"
    if inp["command"] == "translate" and inp.get("nobarcoding") and not inp.get("count_dcrs"):
        return ("--clonotypes with -nbc needs --count-dcrs and a .nbc file: without counts every row would count 1")
    return None


def cdr3_network_refusal(inp: dict):
    """Why the --cdr3-network flags cannot run with these arguments, or None: the network is made of the clonotype table."""
    others = list(inp.get("cdr3_options_given") or []) + (["--write-cdr3-edges"] if inp.get("write_cdr3_edges") else [])
    from .match import WEIGHTED, WEIGHTED_OPTIONS, weighted_refusal
    for key, flag in WEIGHTED_OPTIONS.items():      # (a caller's dictionary names them by key)
        if inp.get(key) is not None and flag not in others:
            others.append(flag)
    if not inp.get("cdr3_network"):
        return f"{', '.join(others)} belong{'s' if len(others) == 1 else ''} to --cdr3-network" if others else None
    if not inp.get("clonotypes"):
        return "--cdr3-network links the rows of the clonotype table: it needs --clonotypes"
    if inp.get("cdr3_distance", 1) not in (1, 2):
        return f"--cdr3-distance is 1 or 2, not {inp['cdr3_distance']}"
    if inp.get("cdr3_class", "v") not in ("none", "v", "vj"):
        return f"--cdr3-class is none, v or vj, not {inp['cdr3_class']}"
    metric = inp.get("cdr3_metric") or "hamming"
    if metric not in ("hamming", "levenshtein", WEIGHTED):
        return f"--cdr3-metric is hamming or levenshtein, or weighted (with --cdr3-radius), not {inp['cdr3_metric']}"
    if metric == WEIGHTED and "--cdr3-distance" in others:
        return "--cdr3-distance does not apply to --cdr3-metric weighted: the radius is --cdr3-radius"
    why = weighted_refusal(dict(inp, cdr3_metric=metric))      # (the four flags without the metric, and their ranges)
    if why:
        return why
    if metric == WEIGHTED and inp.get("cdr3_cost_matrix"):      # a bad matrix file: by its line, before the input is read
        from .match import weighted_settings
        try:
            weighted_settings(dict(inp, cdr3_metric=metric))
        except (ValueError, OSError) as e:
            return str(e)
    return None


def _clonotypes_step(inp: dict):
    """--clonotypes behind cdr3translator: the table (statistics printed and kept), and its file unless dontsave; with
    --cdr3-network the network of its rows behind it, and its files."""
    from . import translate
    from .io import write_out_cdr3_clusters, write_out_cdr3_edges, write_out_clonotypes
    table = translate.clonotypes(inp)
    if inp.get("chain"):
        translate.chain_clonotype_stats[str(inp["chain"]).lower()] = dict(translate.clonotype_stats)
    if not inp.get("dontsave"):
        write_out_clonotypes(table, inp)
    if inp.get("cdr3_network"):
        network = translate.cdr3_network(inp, table)
        if inp.get("chain"):
            translate.chain_cdr3_network_stats[str(inp["chain"]).lower()] = dict(translate.cdr3_network_stats)
        if not inp.get("dontsave"):
            write_out_cdr3_clusters(network, inp)
            if inp.get("write_cdr3_edges"):
                write_out_cdr3_edges(network, inp)
    return table


def collapse_front(data, inp):
    """The rows' front half of `collapse` with the stage's own flags (io.py: -ol, -mq, -bm, -aq, -ln, -N).  Returns the
    FrontRows; prints the reference's counters."""
    collapse.counts.clear()
    params = [inp.get("minbcQ", 20), inp.get("bcQbelowmin", 1), inp.get("avgQthreshold", 30)]       # barcode_quality_parameters (collapse.py:917-921)
    front = collapse.read_in_data(data, inp, params, inp.get("percentlevdist", 10) / 100.0, True, _opener(data) if inp["command"] == "collapse" else None)
    kept = len(front.kept())
    print(f"Collapse front half: {len(front):,} rows in, {kept:,} with a barcode of sufficient quality and an inter-tag sequence within the length threshold")
    for k in sorted(collapse.counts):
        print(f"\t{k},{collapse.counts[k]}")
    return front


def _opener(path):
    import gzip
    return gzip.open if str(path).endswith(".gz") else open


def run(args: Optional[dict[str, Any]] = None, cli_args: Optional[dict[str, Any]] = None):
    inp = cli_args if cli_args else args
    why = clonotype_refusal(dict(inp, command=inp.get("command") or "pipeline"))
    if why:
        raise ValueError(why)
    why = cdr3_network_refusal(inp)
    if why:
        raise ValueError(why)
    if dec.chain_list(inp.get("chain")) is not None:
        return run_chains(inp)
    start = datetime.now()
    data = decombinator(inp)
    return _after_decombine(data, inp, start)


def run_chains(inp: dict) -> dict:
    """`pipeline -c a,b`: the FASTQ decombined once for every chain (decombine.decombinator_chains), then per chain, with
    that chain's arguments, what run() does after decombining.  Returns {chain letter: what run() returns}."""
    start = datetime.now()
    per_chain = dec.decombinator_chains(inp)
    return {chain: _after_decombine(data, _files_args(chain), start) for chain, data in per_chain.items()}


def _files_args(chain: str) -> dict:
    """A chain's arguments of the last decombinator_chains() for what follows the decombine step: the chain as its letter
    (the writers and collapse name files by chainnams[chain], which holds letters; for a list of letters this is the
    chain's own copy as it is)."""
    return dict(dec.chain_args[chain], chain=chain)


def _after_decombine(data, inp, start):
    if inp.get("count_dcrs"):
        # the barcode-free count (-nbc --count-dcrs): the `.nbc`, then translate; no collapse (there are no UMIs)
        from . import translate
        from .io import write_out_translated
        if not inp["dontsave"]:
            write_out_counts(data, inp)
        print("Decombinator complete...")
        if inp.get("clonotypes"):
            inp["clonotype_table"] = getattr(data, "counted", None)      # (the arrays the count read out: translate rebuilds nothing)
        data = translate.cdr3translator(inp, data=data)
        print("CDR3translator complete...")
        if not inp["dontsave"]:
            write_out_translated(data, translate.out_headers, inp)
        if inp.get("clonotypes"):
            _clonotypes_step(inp)
        print(f"Pipeline complete in {datetime.now() - start}")
        return data
    if not inp["dontsave"]:
        write_out_intermediate(data, inp, ".n12")
    print("Decombinator complete...")
    if inp.get("cluster"):
        from . import translate
        from .io import write_out_translated
        inp["clonotype_table"] = None      # (cdr3translator builds it from the rows of the .freq)
        data = collapse.collapsinator(inp, data=data)
        if not inp["dontsave"]:
            write_out_intermediate(data, inp, ".freq")
        print("Collapsinator complete...")
        data = translate.cdr3translator(inp, data=data)
        print("CDR3translator complete...")
        if not inp["dontsave"]:
            write_out_translated(data, translate.out_headers, inp)
        if inp.get("clonotypes"):
            _clonotypes_step(inp)
        print(f"Pipeline complete in {datetime.now() - start}")
        return data
    if len(data) and inp.get("oligo") and not inp.get("nobarcoding"):
        collapse_front(data, inp)
    print("The grouping / clustering half of `collapse` was not asked for: run with --cluster for the .freq and the .tsv.")
    print(f"Pipeline complete in {datetime.now() - start}")
    return data


def main(argv=None):
    inp = cli_args(argv)
    if inp["command"] == "overlap":     # a stage of its own: it reads clonotype tables, not reads
        from . import overlap
        try:
            overlap.run(inp)
        except ValueError as e:
            from .io import create_parser
            create_parser().error(str(e))
        return
    if inp["command"] == "match":       # ... and so is this one: clonotype tables against a database
        from . import match
        try:
            match.run(inp)
        except ValueError as e:
            from .io import create_match_parser
            create_match_parser().error(str(e))
        return
    if inp["command"] == "motifs":      # ... and this one: clonotype tables against a background repertoire
        from . import motifs
        try:
            motifs.run(inp)
        except ValueError as e:
            from .io import create_motifs_parser
            create_motifs_parser().error(str(e))
        return
    if inp["command"] == "metaclonotypes":      # ... and this one: per clonotype a radius from a background repertoire
        from . import metaclonotypes
        try:
            metaclonotypes.run(inp)
        except ValueError as e:
            from .io import create_metaclonotypes_parser
            create_metaclonotypes_parser().error(str(e))
        return
    if inp["command"] == "tabulate":      # ... and this one: meta-clonotypes counted in bulk samples
        from . import tabulate
        try:
            tabulate.run(inp)
        except ValueError as e:
            from .io import create_tabulate_parser
            create_tabulate_parser().error(str(e))
        return
    if inp["command"] == "associate":      # ... and this one: exact tests over a feature by sample table, with a permutation null
        from . import associate
        try:
            associate.run(inp)
        except ValueError as e:
            from .io import create_associate_parser
            create_associate_parser().error(str(e))
        return
    if inp.get("clonotypes"):           # refused before anything is read
        why = clonotype_refusal(inp)
        if why:
            from .io import create_parser
            create_parser().error(why)
    why = cdr3_network_refusal(inp)     # refused before anything is read
    if why:
        from .io import create_parser
        create_parser().error(why)
    if inp.get("merge_errors") or inp.get("write_merges") or inp.get("merge_options_given"):
        from .io import create_parser          # (decombine and pipeline alone take these flags)
        try:
            dec.check_count_args(inp)
        except ValueError as e:
            create_parser().error(str(e))
    if inp.get("count_dcrs"):           # refused before anything is read
        from .io import create_parser
        if inp["command"] == "collapse":
            create_parser().error("--count-dcrs has no collapse step: a barcode-free run has no UMIs to collapse "
                                  "(decombine or pipeline -nbc --count-dcrs write the counts)")
        if inp["command"] != "translate":
            try:
                dec.check_count_args(inp)
            except ValueError as e:
                create_parser().error(str(e))
        elif not inp.get("nobarcoding"):
            create_parser().error("--count-dcrs reads the .nbc of a barcode-free run: it needs -nbc (--nobarcoding)")
    if inp["command"] in ("collapse", "translate") and dec.chain_list(inp.get("chain")) is not None:
        from .io import create_parser
        create_parser().error(f"{inp['command']} works on one per-chain file: -c takes one chain there, not a list "
                              f"({inp['chain']})")
    if inp["command"] in ("decombine", "pipeline") and dec.chain_list(inp.get("chain")) is not None:
        try:
            dec.resolve_chain_list(dec.chain_list(inp["chain"]))      # refused before anything is read
        except ValueError as e:
            from .io import create_parser
            create_parser().error(str(e))

    def write(data, args):
        if args.get("count_dcrs"):
            write_out_counts(data, args)
        else:
            write_out_intermediate(data, args, ".n12")

    if inp["command"] == "decombine" and dec.chain_list(inp.get("chain")) is not None:
        for chain, data in dec.decombinator_chains(inp).items():
            write(data, _files_args(chain))
    elif inp["command"] == "decombine":
        data = decombinator(inp)
        write(data, inp)
    elif inp["command"] == "pipeline":
        run(cli_args=inp)
    elif inp["command"] == "collapse" and inp.get("cluster"):
        # the whole stage (reference pipeline.py:45-47): the `.freq`, named <outpath><file id>.freq
        data = collapse.collapsinator(inp)
        write_out_intermediate(data, inp, ".freq")
    elif inp["command"] == "collapse":
        # the front half over an `.n12` file: the rows that pass, each with its barcode and barcode quality appended
        # (this build's intermediate: the reference goes on to group them in memory)
        front = collapse_front(inp["infile"], inp)
        out = [list(front[k][2]) + [front[k][5], front[k][3], front[k][4], front[k][0], front[k][1]] for k in front.kept().tolist()]
        write_out_intermediate(out, inp, ".n12u")
    elif inp["command"] == "translate":
        # translate.py:388-560 for a `.freq` file: the AIRR `.tsv` (tab-separated, a header line, no index), gzipped unless
        # -dz, mode 666 — the reference's write_out_translated (io.py:516-548)
        from . import translate
        from .io import write_out_translated
        rows = translate.cdr3translator(inp)
        name = write_out_translated(rows, translate.out_headers, inp)
        print("Translated", translate.counts["line_count"], "DCRs,", translate.counts["prod_recomb"], "productive ->", name)
        if inp.get("clonotypes"):
            inp["dontsave"] = False
            _clonotypes_step(inp)
    else:
        from .io import create_parser
        create_parser().print_help()


if __name__ == "__main__":
    main()
