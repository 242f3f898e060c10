"""`python -m vall_e` -- caller of the D3PM sampler with the reference CLI's shape
(/root/reference/vall_e/__main__.py:44-73: TEXT REFERENCE OUT [--ar-ckpt] [--nar-ckpt] [--device]).

Two forms:

    python -m vall_e TEXT REFERENCE.wav OUT.wav [--ar-ckpt zoo/ar.pt] [--nar-ckpt zoo/nar.pt] [--device cuda]

is upstream's command line.  Its front-ends are third-party and need downloads (g2p_en for phonemes, EnCodec for the
prompt and for decoding): they are imported lazily (frontends.py) and a missing one is an error that names it.
The second form takes what those front-ends write (formats.py) and writes what EnCodec's decoder reads:

    python -m vall_e --phn-file utt.phn.txt --symmap symmap.json --prompt-qnt prompt.qnt.pt \
                     --ar-ckpt ar_state_dict.pt --nar-ckpt nar_state_dict.pt out.qnt.pt

  --phonemes    space-separated phoneme ids, or
  --phn-file    a `.phn.txt` file of phone symbols, mapped through `ar.phone_symmap` like upstream (__main__.py:56,61) when
                the checkpoint carries it (state dict key `_symmaps`, or a tools/convert_upstream_pickle.py export), else
                through --symmap (a JSON {symbol: id})
  --prompt-qnt  a `.qnt.pt` file as written by the reference's emb/qnt.py:68,93 (int64 [1, 8, t])
  --nar-ckpt    state_dict of the stock NAR model: levels 1..7 are filled in and `out` is a `.qnt.pt` [1, 8, t];
                without it `out` holds the level-0 codes only ([1, 1, t])
  --frames N    frames to generate (default: the model's n_frames); the `.qnt.pt` that is written holds N frames
  --continue-from FILE.qnt.pt
                level 0 of that file is a known prefix of the utterance: its frames are revealed to the sampler from the
                first iteration on and come back unchanged, the remaining N - prefix frames are generated
  --temperature F, --top-k N
                how sharply the D3PM stage draws: the x0-logits of every reverse step are divided by F (> 0, default 1) and cut
                to their N largest (0 = off, the default; ties kept) before the posterior draw (AR.generate_audio); the NAR stage
                keeps its own sampling_temperature
  --top-p P     nucleus cut behind them (0 < P <= 1, default 1 = off): every draw keeps the smallest set of the largest x0-logits
                that carries the share P of the softmax mass, per row and per step (include/d3pm_hip.h: d3pm_nucleus)
  --reveal-steps N, --choice-temperature F
                run the D3PM stage as a confidence-ordered reveal in N denoiser evaluations (1 .. timesteps - 1; default: the
                timesteps - 1 evaluations of the D3PM loop): every step reveals the frames the model is most sure of; F (>= 0,
                default 0) adds annealed Gumbel noise to that order (include/d3pm_hip.h: d3pm_reveal)
  --revise [BONUS]
                with --reveal-steps: in every step the frames that already hold an id compete again for their place and may be
                re-masked; BONUS (>= 0, default 0 when the flag is bare) is added to a held frame's log-probability before it is
                ranked against the masked frames (include/d3pm_hip.h: d3pm_revise)
  --mask-padding
                the utterance does not attend to its own padding: the keys of every attention are its live frames, its phonemes and
                its prompt frames only (include/d3pm_hip.h: d3pm_keys).  Default off: upstream has the padded rows as keys, and the
                weights were trained that way
  --logprobs PATH
                also save how sure the D3PM stage was of every frame: torch.save({"logprob": float32 [N], "step": int32 [N]}) of the
                N frames written -- the model's log-probability of the id a frame took when it left the mask, and the timestep of that
                evaluation (-1: a frame of the --continue-from prefix; include/d3pm_hip.h: d3pm_frame_scores)
  --nar-top-k N, --nar-top-p P
                the same two cuts for the NAR stage (with --nar-ckpt): every draw of levels 1..7 takes the N largest of its
                logit / sampling_temperature (0 = off, the default; ties kept) and the smallest set of them that carries the share P
                of the mass (default 1 = off; include/d3pm_hip.h: d3pm_nar_draw)
  --nar-guidance W
                classifier-free guidance in the NAR stage (with --nar-ckpt): every draw of levels 1..7 takes rn(fmaf(W, c - u, c)) of
                the frame's logits under the text and the speaker (c) and under the empty text and prompt (u), one evaluation of
                both per level (W >= 0, 0 = off, the default; include/d3pm_hip.h: d3pm_nar_level_guided).  --guidance stays the D3PM
                stage's weight; neither implies the other
  --nar-logprobs PATH
                also save how sure the NAR stage was: torch.save(float32 [N, 7]), column c = the model's log-probability of the
                level c + 1 code of every frame written (of the prefix's own codes under --keep-prefix-levels)
  --keep-prefix-levels
                with --continue-from and --nar-ckpt: all 8 levels of that file are known to the NAR stage, so the first rows of OUT
                are the file's in every level and the recording's sound is kept.  Without it the NAR stage fills levels 1..7 of the
                prefix again, as it always did
"""
import argparse
from pathlib import Path

import torch


def main(argv=None):
    ap = argparse.ArgumentParser("D3PM codec-token sampler (MI355X)")
    ap.add_argument("paths", nargs="+", metavar="[TEXT REFERENCE] OUT",
                    help="OUT.qnt.pt (pre-tokenised form), or upstream's TEXT REFERENCE.wav OUT.wav")
    ap.add_argument("--phonemes", default=None)
    ap.add_argument("--phn-file", type=Path, default=None)
    ap.add_argument("--symmap", type=Path, default=None)
    ap.add_argument("--prompt-qnt", type=Path, default=None)
    ap.add_argument("--ar-ckpt", type=Path, default=None, help="state_dict in the reference key layout (random init if absent)")
    ap.add_argument("--nar-ckpt", type=Path, default=None, help="state_dict of the NAR model (vall_e/vall_e/nar.py)")
    ap.add_argument("--nar-model", default="nar", help="registry name of the NAR model: nar, nar-half, nar-quarter")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16", "float32"])
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--frames", type=int, default=None, help="frames to generate (default: the model's n_frames)")
    ap.add_argument("--continue-from", type=Path, default=None, help=".qnt.pt whose level 0 is the known prefix of the utterance")
    ap.add_argument("--temperature", type=float, default=1.0, help="D3PM stage: divide the x0-logits by this (> 0) before every draw")
    ap.add_argument("--top-k", type=int, default=0, help="D3PM stage: draw from the N largest x0-logits only (0 = off)")
    ap.add_argument("--top-p", type=float, default=1.0, help="D3PM stage: draw from the smallest set of classes that carries this share of the mass (1 = off)")
    ap.add_argument("--reveal-steps", type=int, default=None, help="D3PM stage: confidence-ordered reveal in this many denoiser evaluations")
    ap.add_argument("--choice-temperature", type=float, default=0.0, help="D3PM stage, with --reveal-steps: Gumbel noise on the reveal order (>= 0)")
    ap.add_argument("--revise", type=float, nargs="?", const=0.0, default=None, metavar="BONUS",
                    help="D3PM stage, with --reveal-steps: held frames compete again in every step; BONUS (>= 0, default 0) favours them")
    ap.add_argument("--mask-padding", action="store_true", help="D3PM stage: key-padding masks, the utterance ignores its own padding")
    ap.add_argument("--guidance", type=float, default=0.0, help="D3PM stage: classifier-free guidance weight w (>= 0, 0 = off): draw from (1 + w) cond - w null")
    ap.add_argument("--logprobs", type=Path, default=None, help="D3PM stage: save the per-frame log-probability of the revealed ids and their timesteps here")
    ap.add_argument("--nar-top-k", type=int, default=0, help="NAR stage: draw every level from its N largest logits only (0 = off)")
    ap.add_argument("--nar-top-p", type=float, default=1.0, help="NAR stage: draw from the smallest set of classes that carries this share of the mass (1 = off)")
    ap.add_argument("--nar-guidance", type=float, default=0.0, help="NAR stage: classifier-free guidance weight w (>= 0, 0 = off) in the draw of levels 1..7")
    ap.add_argument("--nar-logprobs", type=Path, default=None, help="NAR stage: save the [frames, 7] log-probabilities of the codes of levels 1..7 here")
    ap.add_argument("--keep-prefix-levels", action="store_true", help="with --continue-from: the prefix's 8 levels are known to the NAR stage")
    ap.add_argument("--native", action="store_true", help="the shape upstream's class really builds (d=32, 16 heads, 8 blocks)")
    args = ap.parse_args(argv)

    from . import formats
    from .vall_e import AR, _hip, get_model
    try:
        _hip.nucleus_options(args.temperature, args.top_k, args.top_p, 1025)
        _hip.reveal_options(args.reveal_steps, args.choice_temperature)
        if _hip.guidance_options(args.guidance) is not None and args.reveal_steps is not None:
            raise ValueError("--guidance does not combine with --reveal-steps")
        if _hip.revise_options(args.revise) is not None and args.reveal_steps is None:
            raise ValueError("--revise needs --reveal-steps")
        _hip.nar_draw_options(args.nar_top_k, args.nar_top_p, 1024)
        if args.keep_prefix_levels and args.continue_from is None:
            raise ValueError("--keep-prefix-levels needs --continue-from")
        nar_guided = _hip.guidance_options(args.nar_guidance) is not None
        nar_flags = args.nar_top_k != 0 or args.nar_top_p != 1.0 or args.nar_logprobs is not None or args.keep_prefix_levels or nar_guided
        if nar_flags and args.nar_ckpt is None:
            raise ValueError("--nar-top-k / --nar-top-p / --nar-guidance / --nar-logprobs / --keep-prefix-levels need --nar-ckpt")
    except ValueError as e:
        ap.error(str(e))
    if len(args.paths) not in (1, 3):
        ap.error("give OUT, or TEXT REFERENCE OUT")
    upstream_form = len(args.paths) == 3
    args.out_path = Path(args.paths[-1])
    if upstream_form:
        if args.phonemes is not None or args.phn_file is not None or args.prompt_qnt is not None:
            ap.error("TEXT REFERENCE OUT takes its phonemes and prompt from TEXT and REFERENCE")
        if args.frames is not None or args.continue_from is not None:
            ap.error("--frames / --continue-from belong to the pre-tokenised form")
        if args.ar_ckpt is None and args.symmap is None:
            ap.error("TEXT needs a phone symmap: an --ar-ckpt that carries ar.phone_symmap, or --symmap")
        from . import frontends
        phones = frontends.g2p_encode(args.paths[0])                                # emb/g2p.py:24-28
        proms = frontends.encodec_encode_file(args.paths[1], args.device)[0].t().contiguous().long().cpu()   # "1 l t -> t l"
    else:
        if (args.phonemes is None) == (args.phn_file is None):
            ap.error("give exactly one of --phonemes / --phn-file")
        if args.phn_file is not None and args.symmap is None and args.ar_ckpt is None:
            ap.error("--phn-file needs a phone symmap: --symmap, or an --ar-ckpt that carries ar.phone_symmap")
        if args.prompt_qnt is None:
            ap.error("--prompt-qnt is required")
        proms = formats.load_quants(args.prompt_qnt)                               # (t, 8) like data.py:31-37

    dtype = getattr(torch, args.dtype)
    model = AR.reference_native().to(args.device) if args.native else get_model("diffusion")
    if args.ar_ckpt is not None:
        blob = torch.load(args.ar_ckpt, map_location="cpu")
        if isinstance(blob, dict) and "state_dict" in blob:                         # tools/convert_upstream_pickle.py export
            model.load_state_dict(blob["state_dict"])
            model.phone_symmap = dict(blob.get("phone_symmap") or {})
            model.spkr_symmap = dict(blob.get("spkr_symmap") or {})
        else:
            model.load_state_dict(blob)
    model = model.to(dtype).to(args.device)
    if upstream_form or args.phn_file is not None:
        symmap = formats.load_symmap(args.symmap) if args.symmap is not None else model.phone_symmap
        if not symmap:
            ap.error("no phone symmap in the checkpoint: give --symmap")
        phones = phones if upstream_form else formats.read_phones(args.phn_file)
        phns = formats.phones_to_ids(phones, symmap)                                # symmap = ar.phone_symmap, __main__.py:56,61
    else:
        phns = torch.tensor([int(p) for p in args.phonemes.split()], dtype=torch.long)
    n_frames = model.cfg.n_frames if args.frames is None else args.frames
    sampling = dict(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, reveal_steps=args.reveal_steps,
                    choice_temperature=args.choice_temperature, mask_padding=args.mask_padding, guidance=args.guidance)
    if args.logprobs is not None:      # (the keyword reaches generate_audio only when the flag is given)
        sampling["return_logprobs"] = True
    if args.revise is not None:
        sampling["revise"] = args.revise
    if args.frames is None and args.continue_from is None:
        codes = model.generate_audio(text_list=[phns], proms_list=[proms], seed=args.seed, **sampling)
    else:
        prefix = None if args.continue_from is None else [formats.load_quants(args.continue_from)[:, 0]]
        codes = model.generate_audio(text_list=[phns], proms_list=[proms], seed=args.seed, n_frames=[n_frames], known=prefix,
                                     **sampling)
    if args.logprobs is not None:
        codes, scores = codes
        torch.save({"logprob": scores.logprob[:n_frames].cpu(), "step": scores.step[:n_frames].cpu()}, args.logprobs)
    resps = codes[:n_frames].unsqueeze(-1)                                         # __main__.py:64 of the reference
    if args.nar_ckpt is not None:
        nar = get_model(args.nar_model)
        nar.load_state_dict(torch.load(args.nar_ckpt, map_location="cpu"))
        nar = nar.to(dtype).to(args.device)
        nar_kw = {}                        # (the keywords reach the NAR model only when their flags are given)
        if args.nar_top_k != 0:
            nar_kw["top_k"] = args.nar_top_k
        if args.nar_top_p != 1.0:
            nar_kw["top_p"] = args.nar_top_p
        if args.keep_prefix_levels:
            full = formats.load_quants(args.continue_from)[:n_frames]                # (t, 8): every level of the prefix
            known = torch.zeros((n_frames, full.shape[1]), dtype=torch.long)
            known[: len(full)] = full
            nar_kw["known"] = [known]
            nar_kw["known_mask"] = [torch.arange(n_frames) < len(full)]
        if nar_guided:
            nar_kw["guidance"] = args.nar_guidance
        if args.nar_logprobs is not None:
            nar_kw["return_logprobs"] = True
        resps = nar(text_list=[phns.to(args.device)], proms_list=[proms.to(args.device)], resps_list=[resps],
                    seed=args.seed, **nar_kw)
        if args.nar_logprobs is not None:
            resps, nar_scores = resps
            torch.save(nar_scores[0].cpu(), args.nar_logprobs)
        resps = resps[0]
    if upstream_form:
        from . import frontends
        frontends.encodec_decode_to_file(resps, args.out_path, args.device)         # qnt.decode_to_file, __main__.py:72
    else:
        formats.save_quants(resps, args.out_path)
    print(args.out_path, "saved.")


if __name__ == "__main__":
    main()
