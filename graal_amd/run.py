"""Headless run from a dataset folder -- what pressing "start" in the reference's GUI does (``main_window.py:617-650`` ->
``simulation_loader.simulation.__init__`` -> ``main_gl.window.start_EM``), without wx / GLUT:

    python -m graal_amd.run --dataset DIR [--fasta genome.fa] --level 3 --cycles 100 --neighbours 3 --out OUT
    python -m graal_amd.run --dataset DIR --size-pyramid 1 --level 0 ...      (restriction-fragment resolution, BASELINE config 4)

DIR holds ``info_contigs.txt``, ``fragments_list.txt``, ``abs_fragments_contacts_weighted.txt`` (``README.md:111-113``).
Steps: build (or reuse) the pyramid, build the sampler inputs of the chosen level, fit the Rippe contact model, run the
MCMC cycles on the MI355X, write the trace files of ``main_gl.py:321-342`` and -- if a FASTA file is given -- the
scaffolded genome (``pyramid_sparse.py:1430-1488``)."""
import argparse
import os
import time

import numpy as np

from . import em
from . import pyramid as pyr


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--fasta", default=None)
    ap.add_argument("--size-pyramid", type=int, default=4)
    ap.add_argument("--factor", type=int, default=3)
    ap.add_argument("--level", type=int, default=3, help="pyramid level of the bins: 1 .. size-pyramid - 1 as in the reference's GUI (main_window.py:452), "
                                                         "or 0 = full restriction-fragment resolution (bins = the filtered level-0 fragments, one "
                                                         "sub-fragment each: what the dense reference cannot run, BASELINE config 4)")
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--neighbours", type=int, default=3)
    ap.add_argument("--blacklist", type=int, nargs="*", default=[0], help="contig ids to blacklist (0 = none)")
    ap.add_argument("--allow-repeats", action="store_true")
    ap.add_argument("--sample-params", action="store_true")
    ap.add_argument("--no-explode", action="store_true")
    ap.add_argument("--seed", type=int, default=None, help="seed of the numpy RandomState (the reference never seeds)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--arithmetic", choices=("strict", "trans_accu", "exact"), default="strict",
                    help="strict = the reference's float32 pixel arithmetic (default: traces are the reference's); exact = "
                         "mathematically exact candidate deltas (faster on long contigs)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", action="store_true", help="write pre_simu.tiff / post_em.tiff (the contact matrix in the genome's order before and after, "
                                                           "main_gl.py:213, 283) into the output folder")
    ap.add_argument("--no-fit", action="store_true", help="skip the Rippe fit; needs --param (8 floats: kuhn lm c1 slope d d_max fact v_inter)")
    ap.add_argument("--param", type=float, nargs=8, default=None, help="param_simu to run with instead of the fit's")
    ap.add_argument("--junctions", action="store_true", help="write junctions.tsv into the output folder: every join of the final layout "
                                                             "with the log-likelihood it carries (graal_amd.junctions)")
    ap.add_argument("--links", action="store_true", help="write links.tsv into the output folder: every pair of contig ends of the final "
                                                         "layout with contacts between them, with the log-likelihood their join would add "
                                                         "(graal_amd.links)")
    ap.add_argument("--links-min-frags", type=int, default=1, help="with --links: only contigs of at least this many fragments (default 1)")
    ap.add_argument("--link-support", type=int, default=0, metavar="R",
                    help="write link_support.tsv into the output folder: links.tsv's columns plus the bootstrap support of every listed "
                         "link of the final layout -- the fraction of R Poisson resamplings of the contacts (1 .. 1024, one GPU call) in "
                         "which the join still scores above 0, the fraction in which it also is the join both ends choose (mutual), and "
                         "the mean, smallest and largest resampled score; --links-min-frags applies")
    ap.add_argument("--link-support-seed", type=int, default=None, help="with --link-support: the seed of the resampling "
                                                                        "(default: --seed, or 0 when that is unset)")
    ap.add_argument("--scaffold", action="store_true", help="after the explode and before the MCMC, join mutual-best contig ends round by "
                                                            "round (graal_amd.scaffold); writes scaffold.tsv")
    ap.add_argument("--scaffold-min-score", type=float, default=0.0, help="with --scaffold: only joins scoring above this (default 0)")
    ap.add_argument("--junction-support", type=int, default=0, metavar="R",
                    help="write junction_support.tsv into the output folder: junctions.tsv's columns plus the bootstrap support of every "
                         "join of the final layout -- the fraction of R Poisson resamplings of the contacts (1 .. 1024, one GPU call) in "
                         "which the join still scores above 0 -- and the mean, smallest and largest resampled score")
    ap.add_argument("--junction-support-seed", type=int, default=None, help="with --junction-support: the seed of the resampling "
                                                                            "(default: --seed, or 0 when that is unset)")
    ap.add_argument("--junction-gaps", action="store_true",
                    help="write junction_gaps.tsv into the output folder: junctions.tsv's columns plus the gap the data estimate at every "
                         "join of the final layout -- the likelihood profile of the gap over a grid, one GPU call: its maximum, the "
                         "interval within --junction-gaps-drop of it, and whether that interval is open towards a cut")
    ap.add_argument("--junction-gaps-points", type=int, default=32, help="with --junction-gaps: grid points, 0 included (2 .. 64, default 32)")
    ap.add_argument("--junction-gaps-max-kb", type=float, default=None, help="with --junction-gaps: the largest gap of the grid in kb "
                                                                             "(default: the model's d_max)")
    ap.add_argument("--junction-gaps-drop", type=float, default=1.92, help="with --junction-gaps: the interval's drop in log-likelihood "
                                                                           "units (default 1.92)")
    ap.add_argument("--polish", action="store_true", help="before the outputs, cut the final layout's junctions scoring below "
                                                          "--polish-cut-below and rejoin the pieces (graal_amd.scaffold); writes polish.tsv")
    ap.add_argument("--polish-cut-below", type=float, default=0.0, help="with --polish: the junction score below which a join is cut (default 0)")
    ap.add_argument("--insert", action="store_true", help="after --scaffold and --polish, before the outputs: put pieces of up to "
                                                          "--insert-max-frags fragments into the junctions they belong to, round by round "
                                                          "(graal_amd.scaffold with insertions); writes insert.tsv")
    ap.add_argument("--insert-max-frags", type=int, default=3, help="with --insert / --insertions: the largest piece, in fragments (default 3)")
    ap.add_argument("--insert-min-score", type=float, default=0.0, help="with --insert: only insertions scoring above this (default 0)")
    ap.add_argument("--flip", action="store_true", help="after --scaffold, --polish and --insert, before the outputs: flip the blocks of up to "
                                                        "--flip-max-frags fragments, and the runs between weak junctions, that the data "
                                                        "prefer the other way round, round by round (graal_amd.flips); writes flip.tsv")
    ap.add_argument("--flip-max-frags", type=int, default=8, help="with --flip / --flips: the longest run of fragments tried (default 8)")
    ap.add_argument("--flip-min-score", type=float, default=0.0, help="with --flip: only flips scoring above this (default 0)")
    ap.add_argument("--flips", action="store_true", help="write flips.tsv into the output folder: every run of up to --flip-max-frags "
                                                         "fragments of the final layout with the log-likelihood its reversal in place "
                                                         "would add, the contacts behind it and a status (graal_amd.flips)")
    ap.add_argument("--swap", action="store_true", help="after --scaffold, --polish and --insert, before --flip: swap the pairs of adjacent runs "
                                                        "of up to --swap-max-frags fragments together, and of runs between weak junctions, "
                                                        "that the data prefer in the other order, round by round (graal_amd.swaps); writes "
                                                        "swap.tsv")
    ap.add_argument("--swap-max-frags", type=int, default=8, help="with --swap / --swaps: the longest pair of runs tried, in fragments (default 8)")
    ap.add_argument("--swap-min-score", type=float, default=0.0, help="with --swap: only swaps scoring above this (default 0)")
    ap.add_argument("--swaps", action="store_true", help="write swaps.tsv into the output folder: every pair of adjacent runs of up to "
                                                         "--swap-max-frags fragments together of the final layout with the log-likelihood "
                                                         "their swap would add, the contacts behind it and a status (graal_amd.swaps)")
    ap.add_argument("--excise", action="store_true", help="after --polish and before --insert: cut the runs of up to --excise-max-frags "
                                                          "fragments, and the runs between weak junctions, that the data prefer out of "
                                                          "their contig, closing the gap behind them, round by round (graal_amd.excise): "
                                                          "the freed pieces are what --insert places; writes excise.tsv")
    ap.add_argument("--excise-max-frags", type=int, default=3, help="with --excise / --excisions: the longest run of fragments tried (default 3)")
    ap.add_argument("--excise-min-score", type=float, default=0.0, help="with --excise: only excisions scoring above this (default 0)")
    ap.add_argument("--excisions", action="store_true", help="write excisions.tsv into the output folder: every run of up to "
                                                             "--excise-max-frags fragments of the final layout with the log-likelihood "
                                                             "cutting it out of its contig would add, the contacts the cut severs and a "
                                                             "status (graal_amd.excise)")
    ap.add_argument("--circularise", action="store_true", help="after --polish, --excise, --insert, --swap and --flip, before the outputs: "
                                                               "close into a ring every linear contig whose ring score is above "
                                                               "--circularise-min-score (graal_amd.rings); the ring model is the "
                                                               "reference's, which prices only pairs less than d_max apart along the "
                                                               "contig; writes circularise.tsv")
    ap.add_argument("--circularise-min-score", type=float, default=0.0, help="with --circularise: only closures scoring above this (default 0)")
    ap.add_argument("--rings", action="store_true", help="write rings.tsv into the output folder: every contig of the final layout with the "
                                                         "log-likelihood closing it into a ring (or, for a ring, opening it at its wrap) "
                                                         "would add, the contacts across the wrap and a status (graal_amd.rings)")
    ap.add_argument("--insertions", action="store_true", help="write insertions.tsv into the output folder: every insertion of a piece of "
                                                              "up to --insert-max-frags fragments into a junction of the final layout that the "
                                                              "contacts support, with the log-likelihood it would add (graal_amd.insert)")
    ap.add_argument("--maps", action="store_true", help="write observed.tiff, expected.tiff, residual.tiff and map_contigs.tsv into the output "
                                                        "folder: the contact matrix of the final layout in genome order, what the model "
                                                        "expects there and their Pearson residual, computed on the GPU (graal_amd.maps)")
    ap.add_argument("--maps-max-px", type=int, default=2048, help="with --maps: the images' largest side, 1 .. 4096 (default 2048)")
    ap.add_argument("--maps-every", type=int, default=0, help="with --maps: also write maps/cycle_%%05d_* behind every C-th cycle (default 0: "
                                                              "the final layout's only)")
    ap.add_argument("--maps-junctions", type=int, default=0, metavar="N",
                    help="write maps/junction_%%03d_{observed,expected,residual}.tiff and maps/map_junctions.tsv into the output folder: "
                         "windows of the three maps around the N junctions of the final layout that the data like least, rendered in one "
                         "call on the GPU (graal_amd.maps)")
    ap.add_argument("--maps-junction-px", type=int, default=256, help="with --maps-junctions: the windows' side in pixels (default 256)")
    ap.add_argument("--maps-junction-bin", type=int, default=1, help="with --maps-junctions: sub-fragments per pixel (default 1)")
    args = ap.parse_args(argv)
    if not 0 <= args.junction_support <= 1024:
        raise SystemExit("--junction-support must be in 0 .. 1024")
    if not 0 <= args.link_support <= 1024:
        raise SystemExit("--link-support must be in 0 .. 1024")
    if args.junction_gaps and (not 2 <= args.junction_gaps_points <= 64 or args.junction_gaps_drop < 0
                               or (args.junction_gaps_max_kb is not None and not args.junction_gaps_max_kb > 0)):
        raise SystemExit("--junction-gaps-points must be in 2 .. 64, --junction-gaps-drop >= 0 and --junction-gaps-max-kb > 0")
    if args.maps_junctions < 0 or (args.maps_junctions and not (1 <= args.maps_junction_px <= 4096 and args.maps_junction_bin >= 1)):
        raise SystemExit("--maps-junctions must be >= 0, --maps-junction-px in 1 .. 4096 and --maps-junction-bin >= 1")
    if args.maps and not 1 <= args.maps_max_px <= 4096:
        raise SystemExit("--maps-max-px must be in 1 .. 4096")
    if not 0 <= args.level < args.size_pyramid:
        raise SystemExit("--level must be in 0 .. size-pyramid - 1 (levels >= 1: the level below holds the observations; 0: the level itself)")
    from .sampler import sampler
    root = os.path.join(args.dataset, "pyramids", "pyramid_%d_thresh_auto" % args.size_pyramid)
    if os.path.exists(os.path.join(root, "pyramid.npz")):
        P = pyr.Pyramid(root, args.size_pyramid)
    else:
        P = pyr.build_and_filter(args.dataset, args.size_pyramid, args.factor)
    inp = pyr.simulation_inputs(P, args.level, candidates_blacklist=args.blacklist, allow_repeats=args.allow_repeats)
    rng = np.random.RandomState(args.seed) if args.seed is not None else None
    smp = sampler(True, inp["S_o_A_frags"], inp["collector_id_repeats"], inp["frag_dispatcher"], inp["id_frag_duplicated"],
                  inp["id_frags_blacklisted"], inp["n_frags"], inp["n_new_frags"], inp["init_n_sub_frags"], inp["n_new_sub_frags"],
                  None, inp["hic_matrix_sub_sampled"], inp["np_sub_frags_len_bp"], inp["np_sub_frags_id"], inp["np_sub_frags_accu"],
                  inp["mean_squared_frags_per_bin"], inp["norm_vect_accu"], inp["S_o_A_sub_frags"], inp["hic_matrix"],
                  inp["mean_value_trans"], args.cycles, False, None, device=args.device, rng=rng,
                  reference_arithmetic=args.arithmetic)
    # simulation_loader.py:109-123: window and bin size of the fit from the initial layout
    g = smp.gpu_vect_frags
    g.copy_from_gpu()
    mean_dist_kb = float(g.l_cont_bp[g.start_bp == 0].mean()) / 1000.0
    size_bin_kb = float(g.len_bp.mean()) / 1000.0
    if args.no_fit:
        if args.param is None:
            raise SystemExit("--no-fit needs --param")
        smp.set_param_simu(np.asarray(args.param, dtype=np.float32))
    else:
        fit_ok = True
        try:
            with np.errstate(all="ignore"):
                smp.estimate_parameters(mean_dist_kb, size_bin_kb)
            fit_ok = bool(np.all(np.isfinite(smp._param_flat)))
        except Exception as e:      # (graal_set_params refuses parameters that are not finite / out of range)
            fit_ok = False
            print("graal_amd.run: the Rippe fit of this dataset gave no usable parameters (%s)" % e)
        if args.param is not None:
            smp.set_param_simu(np.asarray(args.param, dtype=np.float32))
        elif not fit_ok:
            # the reference would carry on with whatever leastsq returned (optim_rippe_curve_update.py:93-115) and score NaN from the first
            # step on; a headless run says so instead
            raise SystemExit("graal_amd.run: the Rippe fit did not converge to finite parameters on this dataset (histogram of %d distance bins, "
                             "%d of them without contacts): pass --param kuhn lm c1 slope d d_max fact v_inter" % (
                                 len(smp.bins), int(np.sum(np.asarray(smp.mean_contacts) <= 1e-10))))
    out = args.out or os.path.join(args.dataset, "graal_out")
    os.makedirs(out, exist_ok=True)
    images = (os.path.join(out, "pre_simu.tiff"), os.path.join(out, "post_em.tiff")) if args.images else None
    t0 = time.perf_counter()
    scrambled = not args.no_explode
    if args.scaffold:
        from . import scaffold
        if scrambled:
            smp.explode_genome()
        scaffold.write_scaffold_tsv(os.path.join(out, "scaffold.tsv"), scaffold.scaffold(smp, min_score=args.scaffold_min_score))
        scrambled = False
    on_cycle = None
    if args.maps and args.maps_every > 0:
        from . import maps

        def on_cycle(j, s):
            if (j + 1) % args.maps_every == 0:
                maps.write_maps(os.path.join(out, "maps"), "cycle_%05d_" % j, maps.layout_maps(s, args.maps_max_px))
    trace = em.run_em(smp, args.cycles, args.neighbours, rng=rng, sample_param=args.sample_params, scrambled=scrambled,
                      matrix_files=images, on_cycle=on_cycle)
    dt = time.perf_counter() - t0
    em.save_behaviour_to_txt(trace, out)
    if args.polish:
        from . import scaffold
        scaffold.write_scaffold_tsv(os.path.join(out, "polish.tsv"), scaffold.scaffold(smp, cut_below=args.polish_cut_below))
    if args.excise:
        from . import excise
        excise.write_excise_rounds_tsv(os.path.join(out, "excise.tsv"),
                                       excise.excise_rounds(smp, max_frags=args.excise_max_frags, min_score=args.excise_min_score))
    if args.insert:
        from . import scaffold
        scaffold.write_scaffold_tsv(os.path.join(out, "insert.tsv"),
                                    scaffold.scaffold(smp, insert_max_frags=args.insert_max_frags, insert_min_score=args.insert_min_score))
    if args.swap:
        from . import swaps
        swaps.write_swap_rounds_tsv(os.path.join(out, "swap.tsv"),
                                    swaps.swap_rounds(smp, max_frags=args.swap_max_frags, min_score=args.swap_min_score))
    if args.flip:
        from . import flips
        flips.write_flip_rounds_tsv(os.path.join(out, "flip.tsv"),
                                    flips.flip_rounds(smp, max_frags=args.flip_max_frags, min_score=args.flip_min_score))
    if args.circularise:
        from . import rings
        rings.write_close_rings_tsv(os.path.join(out, "circularise.tsv"), rings.close_rings(smp, min_score=args.circularise_min_score))
    lev = P.get_level(args.level)
    if args.fasta:
        P.load_reference_sequence(args.fasta)
        g.copy_from_gpu()
        lev.generate_new_fasta(g, os.path.join(out, "genome.fasta"), os.path.join(out, "info_frags.txt"))
    if args.junctions:
        from . import junctions
        junctions.write_junctions_tsv(os.path.join(out, "junctions.tsv"), junctions.junction_table(smp))
    if args.junction_support:
        from . import junctions
        boot_seed = args.junction_support_seed if args.junction_support_seed is not None else (args.seed if args.seed is not None else 0)
        junctions.write_support_tsv(os.path.join(out, "junction_support.tsv"),
                                    junctions.support_table(smp, boot_seed, args.junction_support))
    if args.junction_gaps:
        from . import junctions
        junctions.write_gaps_tsv(os.path.join(out, "junction_gaps.tsv"),
                                 junctions.gap_table(smp, None, args.junction_gaps_drop, args.junction_gaps_points, args.junction_gaps_max_kb))
    if args.links:
        from . import links
        links.write_links_tsv(os.path.join(out, "links.tsv"), links.link_table(smp, args.links_min_frags))
    if args.link_support:
        from . import links
        boot_seed = args.link_support_seed if args.link_support_seed is not None else (args.seed if args.seed is not None else 0)
        links.write_support_tsv(os.path.join(out, "link_support.tsv"),
                                links.support_table(smp, boot_seed, args.link_support, args.links_min_frags))
    if args.insertions:
        from . import insert
        table, _ = insert.fitting_insertion_table(smp, args.insert_max_frags)   # (a smaller piece size when over the device budget)
        if table is not None:
            insert.write_insertions_tsv(os.path.join(out, "insertions.tsv"), table)
    if args.flips:
        from . import flips, scaffold
        eng = scaffold._engine(smp)
        soa = eng.download_frags()
        flips.write_flips_tsv(os.path.join(out, "flips.tsv"), flips.score_table(eng, soa, flips.tilings(soa, None, args.flip_max_frags)))
    if args.swaps:
        from . import scaffold, swaps
        eng = scaffold._engine(smp)
        soa = eng.download_frags()
        swaps.write_swaps_tsv(os.path.join(out, "swaps.tsv"), swaps.score_table(eng, soa, swaps.tilings(soa, None, args.swap_max_frags)))
    if args.excisions:
        from . import excise, scaffold
        eng = scaffold._engine(smp)
        soa = eng.download_frags()
        excise.write_excisions_tsv(os.path.join(out, "excisions.tsv"),
                                   excise.score_table(eng, soa, excise.tilings(soa, None, args.excise_max_frags)))
    if args.rings:
        from . import rings, scaffold
        rings.write_rings_tsv(os.path.join(out, "rings.tsv"), rings.ring_table(scaffold._engine(smp)))
    if args.maps:
        from . import maps
        maps.write_maps(out, "", maps.layout_maps(smp, args.maps_max_px))
    if args.maps_junctions:
        from . import junctions, maps, scaffold
        eng = scaffold._engine(smp)
        soa = eng.download_frags()
        score, _ = eng.junction_scores()
        origins, table = maps.junction_windows(junctions.table_from(soa, score), soa, eng.sub_id, maps.rank_of_sub(soa, eng.sub_id),
                                               args.maps_junctions, args.maps_junction_px, args.maps_junction_bin)
        if len(origins):      # (a layout without a scored junction has nothing to show)
            maps.write_junction_maps(os.path.join(out, "maps"),
                                     maps.window_maps(eng, origins, args.maps_junction_px, bin=args.maps_junction_bin), table)
    n_steps = len(trace.likelihood)
    print("%d bins (%d fragments, %d sub-fragments), %d MCMC steps in %.1f s (%.0f us/step): %d contigs, logL %.6e, "
          "distance to the initial genome %.4f; traces in %s" % (inp["n_frags"], inp["n_new_frags"], inp["init_n_sub_frags"], n_steps,
                                                                 dt, 1e6 * dt / max(n_steps, 1), trace.n_contigs[-1],
                                                                 trace.likelihood[-1], trace.dist[-1], out))
    smp.free_gpu()
    return trace


if __name__ == "__main__":
    main()
