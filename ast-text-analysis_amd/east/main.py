# -*- coding: utf-8 -*-
"""`east` CLI, table branch (reference east/main.py:15-122 as documented in
README.rst:27-63; the shipped reference main crashes with a NameError).

    east [-s ast] [-a easa|easa_hip|ast_linear|ast_naive] [-d] [-f xml|csv] \\
         keyphrases table <keyphrases file> <directory with .txt files | single file>
    east [-c confidence] [-r relevance] [-p support] [-f edges|gml] keyphrases graph <keyphrases file> <texts>
    east [-n N] [-b text|keyphrase] [-r threshold] [-f xml|csv] keyphrases top <keyphrases file> <texts>
        the N (default 10, at most 1024) best keyphrases of every text (-b text, the default) or the N best texts of every
        keyphrase, best first, selected on the device (csrc/top.h); -r: only scores that reach it (default: no threshold)
    east [-n N] [-b text|keyphrase] [-r threshold] [-f xml|csv] keyphrases similar <keyphrases file> <texts>
        the N texts most like every text (-b text: the cosine of their keyphrase profiles, the columns of the score table) or
        the N keyphrases most like every keyphrase (-b keyphrase: of their text profiles, the rows), best first, matrix and
        ranking on the device (csrc/similarity.h); -r: only similarities that reach it (default: no threshold)
    east [-n N] [-r threshold] [-o symmetric|directed] [-d] [-f xml|csv] texts related <directory with .txt files | single file>
        the N texts most related to every text, from the texts alone (no keyphrase file): every string of text A is scored
        against the tree of text B out of the index, the scores are averaged per A (-o directed) and with the opposite
        direction (-o symmetric, the default), best first, on the device (csrc/related.h); one device, the AST measure
    east [-w tf|tf-idf] [-v stems|words] [-n N] [-r threshold] [-l language] [-f xml|csv] texts similar <directory | single file>
        the N texts most like every text, from the texts alone: the cosine of their tf or tf-idf term vectors (the cosine
        measure's own index, stopwords and stemmer), best first, matrix and ranking on the device (csrc/cosine_texts.h); one
        device; `-s ast` is refused (that question is `texts related`)
    east [-s ast|cosine] [-j single|complete|average] [-r threshold | -k clusters] [-w tf|tf-idf] [-v stems|words] [-d]
         [-f xml|csv|merges] texts clusters <texts>
        the groups the texts fall into: single-linkage clusters of the symmetric relatedness (-s ast, the default) or of the
        term-vector cosine (-s cosine), built where the matrix lies (csrc/clusters.h); -r: the texts joined by similarities
        that reach it, -k: that many clusters, one of the two -- or neither with -f merges, the dendrogram a merge a line;
        -j complete / -j average: those linkages, in rounds of reciprocal strongest pairs on a working copy of the matrix
        (csrc/linkage.h) -- -r is then also the floor below which no merge is made: -f merges ends there
    east [-w tf|tf-idf] [-v stems|words] [-n N] [-u min texts] [-l language] [-f xml|csv] texts terms <texts>
        what every text is about: its N (default 10, at most 1024) characteristic terms, the words or stems with the largest
        tf or tf-idf weight over the text's norm, best first, summed and ranked on the device (csrc/terms.h)
    east [-j linkage] (-r threshold | -k clusters) [-w ..] [-v ..] [-n N] [-u min texts] [-f xml|csv] texts terms <texts>
        the same of every cluster `texts clusters -s cosine` finds with that linkage and cut, on the same index: the terms
        with the largest mean over the cluster's texts among those that -u (default 1) of them hold
    east [-x words] [-o symmetric|directed] [-n N] [-r threshold] [-l language] [-f xml|csv] texts overlap <texts>
        the N texts every text shares most WORDING with -- near-duplicates, lifted passages, quotations: a text is the set
        of its shingles of -x (default 4, at most 8) consecutive words; -o symmetric: the resemblance |A n B| / |A u B|,
        -o directed: the containment |A n B| / |A| of the listing text in the listed one; exact integers and one division,
        on the device (csrc/overlap.h); with -j single|complete|average and (-r threshold | -k clusters | -f merges) the
        clusters of the symmetric matrix instead -- single linkage at a resemblance threshold: the near-duplicate groups
    east [-x words] [-m min words] [-k passages per pair] [-n N] [-r threshold] [-o symmetric|directed] [-l language]
         [-f xml|csv] texts passages <texts>
        WHICH words they share: for every text and each of the N texts `texts overlap` ranks for it (same -x, -o, -r) the
        passages of the text in which every -x (default 4, at most 8) consecutive words occur in the other, the longest
        first; -m: only passages of that many words or more (default: -x); -k: that many passages a pair at most (default
        5, 0 = all); per passage where it starts in the text, its words, and where its first -x words first start in the
        other (positions count the words of 3 code points or more from 0); exact integers, on the device (csrc/passages.h)
    east [-s ast|cosine|bm25] [-j linkage] [-b text|keyphrase] [-r threshold | -k clusters] [-f xml|csv|merges] keyphrases clusters <keyphrases file> <texts>
        the same of the texts (-b text) or the keyphrases (-b keyphrase) by the profile cosines of `keyphrases similar`
    east [-n N] [-x max words] [-m min count] [-u min texts] [-l language] [-f txt|csv|xml] keyphrases extract <texts>
        keyphrase candidates out of the texts themselves (no keyphrase file): the repeated phrases of one to -x (default 3, at
        most 8) words that occur -m (default 2) times or more in -u (default 1) texts or more, without those that only ever
        occur inside one longer phrase, by count x words, best first; -n: that many (default 100, 0 = all); the words are
        the cosine measure's (at least 3 code points, its stopwords break a phrase), counted on the device (csrc/phrases.h);
        -f txt (the default) is a keyphrase file: east keyphrases extract texts > kp.txt; east keyphrases top kp.txt texts
    east -s cosine [-w tf|tf-idf] [-v stems|words] keyphrases table|graph|top|similar|clusters ...
        the cosine measure (relevance.CosineRelevanceMeasure) on one device; `-v stems` (the default) needs nltk's
        Snowball stemmer, and without nltk's stopword list no stopwords are removed (said on stderr)
    east -s bm25 [-v stems|words] [-z k1,b] keyphrases table|graph|top|similar|clusters ...
        Okapi BM25 (relevance.BM25RelevanceMeasure) as a second score call of the cosine measure's term index, on one
        device: its tokens, stopwords and stemmer; -z: k1 >= 0 and 0 <= b <= 1 (default 1.2,0.75); -w belongs to cosine
    east -y -t <triples file> keyphrases table|graph ...
        synonym extraction (synonyms.SynonymExtractor, reference main.py:104-133) from dependency triples made elsewhere:
        Tomita's XML output, or lines of w1<TAB>relation<TAB>w2; one device; -y without -t is refused (no parser here)

Several GPUs (one process per GPU, documents sharded over the ranks, one RCCL all-gather of the score blocks --
east/parallel.py; the reference's loops relevance.py:41-53 / applications.py:43-52 are what is sharded):
    east -g 8 keyphrases table ...          or   EAST_HIP_DEVICES=8 east keyphrases table ...
        starts the 8 ranks itself (child processes under torch.distributed.run) and relays rank 0's output;
    python -m torch.distributed.run --nproc-per-node 8 ... -m east.main keyphrases table ...
        under a launcher (WORLD_SIZE > 1 in the environment) every rank runs this module, rank 0 prints.
"""
import getopt
import os
import sys

from east import applications
from east import consts
from east import exceptions
from east import formatting
from east import relevance


def _read(path):
    with open(path, "rb") as f:
        return f.read()


_OPTIONS = "s:a:w:v:l:f:c:r:p:g:t:n:b:o:k:x:m:u:z:j:dy"
_VALUE_OPTIONS = frozenset(c for c, nxt in zip(_OPTIONS, _OPTIONS[1:] + " ") if nxt == ":")


def _world():
    """(world size, rank) a launcher gave this process (torch.distributed.run exports both)."""
    return int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))


def launch_ranks(n_ranks, argv):
    """The no-launcher spelling of a multi-GPU run (`-g N` / EAST_HIP_DEVICES=N): start N ranks of this module as
    CHILD processes under torch.distributed.run (east/launch.py), let their output through (only rank 0 prints) and
    return their exit code.  Nothing in this process has touched a GPU at this point, and it never exec()s.
    EAST_HIP_LAUNCHER replaces the launcher command (tests)."""
    from east import launch
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (the ranks must not start ranks of their own, and every rank takes the device of its LOCAL_RANK)
    return launch.run_ranks(n_ranks, ["-m", "east.main"] + list(argv), "EAST_HIP_LAUNCHER",
                            env_drop=("EAST_HIP_DEVICES", "EAST_HIP_DEVICE"), pythonpath=pkg)


def main(argv=None, measure_factory=None):
    """measure_factory: test hook of the multi-rank path (the per-shard scorer of DistributedASTRelevanceMeasure;
    the collective logic then runs on gloo without a GPU)."""
    args = sys.argv[1:] if argv is None else list(argv)
    try:
        opts, args = getopt.getopt(args, _OPTIONS)
    except getopt.GetoptError as e:
        print(e)
        return 1
    opt_list = opts                                         # (as given: repeated options, empty values)
    opts = dict(opts)
    world, rank = _world()
    refusal = _linkage_refusal(opts, args) or _bm25_refusal(opts, args, world)     # (before a rank is started, a file is read or anything touches the device)
    if refusal:
        if rank == 0:
            print(refusal)
        return 1
    if args[:2] in (["keyphrases", "top"], ["keyphrases", "similar"]):
        # (-n, -b, -r: refused here, before a rank is started, a file is read or anything touches the device)
        refusal = _top_options(opts)[3]
        if refusal:
            if rank == 0:
                print(refusal)
            return 1
    if args[:1] == ["texts"]:
        return _texts_main(opts, args, world, rank)
    if args[:2] == ["keyphrases", "clusters"]:
        return _clusters_main(opts, args, world, rank)
    if args[:2] == ["keyphrases", "extract"]:
        return _extract_main(opts, args, world, rank)
    cosine = opts.get("-s", "").lower() == consts.RelevanceMeasure.COSINE
    if world > 1 and cosine:
        if rank == 0:
            print("Relevance measure 'cosine' runs on one device: a launcher with WORLD_SIZE=%d is not supported." % world)
        return 1
    with_synonyms = "-y" in opts and "-t" in opts            # (-y alone ends in _main with the line it always printed)
    if world > 1 and with_synonyms:
        if rank == 0:
            print("Synonym extraction (-y) runs on one device: a launcher with WORLD_SIZE=%d is not supported." % world)
        return 1
    if world == 1:
        try:
            n_ranks = int(opts.get("-g", os.environ.get("EAST_HIP_DEVICES", "1")))
        except ValueError:
            print("Invalid number of GPUs: '%s'." % opts.get("-g", os.environ.get("EAST_HIP_DEVICES")))
            return 1
        if n_ranks > 1 and cosine:
            # (several devices would need an all-reduce of the document frequencies)
            print("Relevance measure 'cosine' runs on one device: -g %d is not supported." % n_ranks)
            return 1
        if n_ranks > 1 and with_synonyms:
            print("Synonym extraction (-y) runs on one device: -g %d is not supported." % n_ranks)
            return 1
        if n_ranks > 1 and os.environ.get("EAST_HIP_MULTI", "threads") != "process":
            # the default: N devices in THIS process (one AST shard and one host thread of the library per device, one
            # RCCL all-gather of the score blocks -- east_hip_score_table_multi); no child processes, no torch
            opts["-g"] = str(n_ranks)
        elif n_ranks > 1:
            # EAST_HIP_MULTI=process: one process per GPU under torch.distributed.run --
            # the same command line without -g: the ranks learn the world size from the launcher
            child_argv = []
            for key, value in opt_list:
                if key != "-g":
                    child_argv.extend([key, value] if key[1:] in _VALUE_OPTIONS else [key])
            child_argv.extend(args)
            return launch_ranks(n_ranks, child_argv)
    quiet = rank != 0                                       # under a launcher only rank 0 prints
    opts.setdefault("-l", consts.Language.ENGLISH)
    opts.setdefault("-s", consts.RelevanceMeasure.AST)
    opts.setdefault("-a", consts.ASTAlgorithm.EASA)

    saved_stdout = sys.stdout
    if quiet:
        sys.stdout = open(os.devnull, "w")
    try:
        return _main(opts, args, world, measure_factory)
    finally:
        if quiet:
            sys.stdout.close()
            sys.stdout = saved_stdout


def _main(opts, args, world, measure_factory):
    if len(args) < 2:
        print("Invalid syntax: EAST should be called as:\n\n"
              "    east [options] <command> <subcommand> args\n\n"
              "Commands available: keyphrases, texts.\n"
              "Subcommands available: table/graph/top/similar/clusters/extract; related/similar/clusters/terms.")
        return 1

    command, subcommand = args[0], args[1]
    if command != "keyphrases":
        print("Invalid command: '%s'. Please use one of: 'keyphrases', 'texts'." % command)
        return 1
    if len(args) < 4:
        print('Invalid syntax. For keyphrases analysis, EAST should be called as:\n\n'
              '    east [options] keyphrases <subcommand> "path/to/keyphrases.txt" '
              '"path/to/texts/dir"')
        return 1

    keyphrases = _read(os.path.abspath(args[2])).decode("utf-8", errors="replace").splitlines()   # main.py:60-64

    text_collection_path = os.path.abspath(args[3])                                             # main.py:67-89
    if os.path.isdir(text_collection_path):
        text_files = [os.path.join(text_collection_path, filename)
                      for filename in sorted(os.listdir(text_collection_path)) if filename.endswith(".txt")]
    else:
        text_files = [text_collection_path]
    distributed = world > 1 or os.environ.get("EAST_HIP_FORCE_DIST") == "1"
    texts = {}
    if len(text_files) == 1:      # a single file: one text per line
        lines = _read(text_files[0]).splitlines()
        for i in range(len(lines)):
            texts[str(i)] = lines[i]
    elif distributed:
        # one rank per GPU: the documents are sharded by their FILE SIZES (os.stat); a rank reads its own files only
        from east import parallel
        for filename in text_files:
            texts[os.path.basename(filename)[:-4]] = parallel.LazyText(filename, _read)
    else:
        for filename in text_files:
            texts[os.path.basename(filename)[:-4]] = _read(filename)

    measure_name = opts["-s"]
    cosine = measure_name.lower() == consts.RelevanceMeasure.COSINE
    bm25 = measure_name.lower() == consts.RelevanceMeasure.BM25
    if measure_name.lower() != "ast" and not cosine and not bm25:
        print("Relevance measure '%s' is not available (use 'ast', 'cosine' or 'bm25')." % measure_name)
        return 1
    if "-y" in opts and "-t" not in opts:
        print("Synonym extraction (-y) needs the external Tomita parser and is not available.")
        return 1
    if "-t" in opts and "-y" not in opts:
        print("Option -t names the dependency triples of synonym extraction: use it with -y.")
        return 1
    synonimizer = None
    if "-y" in opts:                                                                            # main.py:104-106
        if distributed:
            print("Synonym extraction (-y) runs on one device: the collective path is not supported.")
            return 1
        try:
            from east import synonyms
            synonimizer = synonyms.SynonymExtractor(text_collection_path, triples=os.path.abspath(opts["-t"]))
        except (exceptions.EastException, EnvironmentError) as e:
            print(e)
            return 1
    if cosine:
        if distributed:
            print("Relevance measure 'cosine' runs on one device: the collective path is not supported.")
            return 1
        return _run_cosine(subcommand, keyphrases, texts, opts, synonimizer)
    if bm25:                                                # (the collective path was refused in main)
        return _run_bm25(subcommand, keyphrases, texts, opts, synonimizer)

    group_up = False
    try:
        if distributed:                                                   # (forced: the collective path with one rank)
            # one rank per GPU: this rank indexes its share of the documents on the device of its LOCAL_RANK and
            # the K x D table is assembled by one all-gather (east/parallel.py); every rank computes, rank 0 prints
            import torch.distributed as dist
            from east import parallel
            backend = os.environ.get("EAST_HIP_DIST_BACKEND", "nccl")      # (gloo: the CPU-tier tests)
            if not dist.is_initialized():
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                kwargs = {}
                if backend == "nccl":
                    import torch
                    local = int(os.environ.get("LOCAL_RANK", "0"))
                    torch.cuda.set_device(local)
                    kwargs["device_id"] = torch.device("cuda", local)
                dist.init_process_group(backend, **kwargs)
                group_up = True
            device = int(os.environ.get("LOCAL_RANK", "0")) if backend == "nccl" else None
            similarity_measure = parallel.DistributedASTRelevanceMeasure(opts["-a"], "-d" not in opts, device=device,
                                                                         measure_factory=measure_factory, table_rank=0)
        elif world == 1 and int(opts.get("-g", "1")) > 1:
            similarity_measure = relevance.MultiDeviceASTRelevanceMeasure(opts["-a"], "-d" not in opts, int(opts["-g"]))
        else:
            similarity_measure = relevance.ASTRelevanceMeasure(opts["-a"], "-d" not in opts)      # main.py:95-98
        return _run(subcommand, keyphrases, texts, similarity_measure, opts, synonimizer)
    except exceptions.EastException as e:       # (no device, a failed build ...): a message, not a traceback
        print(e)
        return 1
    finally:
        if group_up:
            import torch.distributed as dist
            dist.destroy_process_group()


def _read_texts(path):
    """{text name: text} of a directory of .txt files (the name: the file's without .txt) or of a single file (a text a
    line, named by its number), as _main reads them (main.py:67-89)."""
    path = os.path.abspath(path)
    if os.path.isdir(path):
        text_files = [os.path.join(path, filename) for filename in sorted(os.listdir(path)) if filename.endswith(".txt")]
    else:
        text_files = [path]
    texts = {}
    if len(text_files) == 1:      # a single file: one text per line
        lines = _read(text_files[0]).splitlines()
        for i in range(len(lines)):
            texts[str(i)] = lines[i]
    else:
        for filename in text_files:
            texts[os.path.basename(filename)[:-4]] = _read(filename)
    return texts


def _related_options(opts):
    """(n, orientation, threshold, None) of `texts related`, or (None, None, None, the one line that says what is wrong)."""
    n, _, threshold, refusal = _top_options({key: value for key, value in opts.items() if key != "-b"})
    if refusal:
        return None, None, None, refusal.replace("relevance threshold", "relatedness threshold")
    orientation = opts.get("-o", "symmetric").lower()
    if orientation not in ("symmetric", "directed"):
        return None, None, None, "Invalid orientation: '%s'. Please use one of: 'symmetric', 'directed'." % opts["-o"]
    return n, orientation, threshold, None


def _texts_main(opts, args, world, rank):
    """`east texts related <texts>` (and `east texts similar <texts>`: _texts_similar_main; `east texts terms <texts>`:
    _texts_terms_main).  Everything that cannot be done is refused with one line before a file is read or
    anything touches a device."""
    def refuse(line):
        if rank == 0:
            print(line)
        return 1

    if len(args) < 2 or args[1] not in ("related", "similar", "clusters", "terms", "overlap", "passages"):
        return refuse("Invalid subcommand: '%s'. Please use one of: 'related', 'similar', 'clusters', 'terms', 'overlap', 'passages'." % (args[1] if len(args) > 1 else ""))
    if args[1] == "overlap":
        return _texts_overlap_main(opts, args, world, refuse)
    if args[1] == "passages":
        return _texts_passages_main(opts, args, world, refuse)
    if args[1] == "similar":
        return _texts_similar_main(opts, args, world, refuse)
    if args[1] == "terms":
        return _texts_terms_main(opts, args, world, refuse)
    if args[1] == "clusters":
        return _clusters_main(opts, args, world, rank)
    if len(args) < 3:
        return refuse('Invalid syntax. For text analysis, EAST should be called as:\n\n'
                      '    east [options] texts related "path/to/texts/dir"')
    n, orientation, threshold, refusal = _related_options(opts)
    if refusal:
        return refuse(refusal)
    if opts.get("-s", consts.RelevanceMeasure.AST).lower() != consts.RelevanceMeasure.AST.lower():
        return refuse("Text relatedness is defined by the AST measure: -s %s is not supported." % opts["-s"])
    if "-y" in opts:
        return refuse("Text relatedness takes no synonyms: -y is not supported.")
    if world > 1:
        return refuse("Text relatedness runs on one device: a launcher with WORLD_SIZE=%d is not supported." % world)
    if os.environ.get("EAST_HIP_FORCE_DIST") == "1":
        return refuse("Text relatedness runs on one device: the collective path is not supported.")
    devices = opts.get("-g", os.environ.get("EAST_HIP_DEVICES", "1"))
    try:
        n_ranks = int(devices)
    except ValueError:
        return refuse("Invalid number of GPUs: '%s'." % devices)
    if n_ranks > 1:
        return refuse("Text relatedness runs on one device: -g %d is not supported." % n_ranks)
    texts = _read_texts(args[2])
    try:
        measure = relevance.ASTRelevanceMeasure(opts.get("-a", consts.ASTAlgorithm.EASA), "-d" not in opts)
        related = applications.texts_related(texts, n, orientation, threshold, measure, opts.get("-l", consts.Language.ENGLISH))
        print(formatting.format_related(related, opts.get("-f", "xml").lower()))
    except exceptions.EastException as e:       # (no device, a failed build ...): a message, not a traceback
        print(e)
        return 1
    except Exception as e:                      # (an unknown format)
        print(e)
        return 1
    return 0


def _texts_similar_main(opts, args, world, refuse):
    """`east texts similar <texts>`: the cosine of the texts' term vectors.  Everything that cannot be done is refused with one
    line (refuse) before a file is read or a measure is made."""
    if len(args) < 3:
        return refuse('Invalid syntax. For text analysis, EAST should be called as:\n\n'
                      '    east [options] texts similar "path/to/texts/dir"')
    n, _, threshold, refusal = _top_options({key: value for key, value in opts.items() if key != "-b"})
    if refusal:
        return refuse(refusal.replace("relevance threshold", "similarity threshold"))
    measure_name = opts.get("-s", consts.RelevanceMeasure.COSINE).lower()
    if measure_name == consts.RelevanceMeasure.AST.lower():
        return refuse("Text similarity is the cosine of term vectors: -s %s is not supported (see `texts related`)." % opts["-s"])
    if measure_name != consts.RelevanceMeasure.COSINE:
        return refuse("Relevance measure '%s' is not available for `texts similar` (use 'cosine')." % opts["-s"])
    if opts.get("-v", consts.VectorSpace.STEMS).lower() == consts.VectorSpace.LEMMATA:
        return refuse("Text similarity has no lemmatizer: -v %s is not supported (use 'stems' or 'words')." % opts["-v"])
    if "-y" in opts:
        return refuse("Text similarity takes no synonyms: -y is not supported.")
    if "-o" in opts:
        return refuse("Text similarity is symmetric: -o %s is not supported (an orientation belongs to `texts related`)." % opts["-o"])
    if world > 1:
        return refuse("Text similarity runs on one device: a launcher with WORLD_SIZE=%d is not supported." % world)
    if os.environ.get("EAST_HIP_FORCE_DIST") == "1":
        return refuse("Text similarity runs on one device: the collective path is not supported.")
    devices = opts.get("-g", os.environ.get("EAST_HIP_DEVICES", "1"))
    try:
        n_ranks = int(devices)
    except ValueError:
        return refuse("Invalid number of GPUs: '%s'." % devices)
    if n_ranks > 1:
        return refuse("Text similarity runs on one device: -g %d is not supported." % n_ranks)
    try:
        measure = relevance.CosineRelevanceMeasure(opts.get("-v", consts.VectorSpace.STEMS), opts.get("-w", consts.TermWeighting.TF_IDF))
        if measure.stopwords_source == "none":
            sys.stderr.write("nltk's English stopword list is not available: no stopwords are removed.\n")
        texts = _read_texts(args[2])
        similar = applications.texts_similar(texts, n, threshold, measure, opts.get("-l", consts.Language.ENGLISH))
        print(formatting.format_similar(similar, "text", opts.get("-f", "xml").lower()))
    except exceptions.EastException as e:       # (a missing stemmer, no device, a failed build ...): a message, not a traceback
        print(e)
        return 1
    except Exception as e:                      # (an unknown format)
        print(e)
        return 1
    return 0


def _texts_overlap_main(opts, args, world, refuse):
    """`east texts overlap <texts>`: the texts that share wording, by their sets of -x word shingles; with -j the clusters of
    the symmetric matrix.  Everything that cannot be done is refused with one line (refuse) before a file is read or a measure
    is made."""
    if len(args) < 3:
        return refuse('Invalid syntax. For text analysis, EAST should be called as:\n\n'
                      '    east [options] texts overlap "path/to/texts/dir"')
    for key, line in (("-s", "Shingle overlap compares wording, not a relevance measure: -s %s is not supported."),
                      ("-w", "Shingle overlap weighs no terms: -w %s is not supported."),
                      ("-v", "Shingles are made of words: -v %s is not supported."),
                      ("-y", "Shingle overlap takes no synonyms: -y is not supported."),
                      ("-b", "Shingle overlap compares texts: -b %s is not supported."),
                      ("-c", "Shingle overlap builds no graph: -c %s is not supported."),
                      ("-p", "Shingle overlap builds no graph: -p %s is not supported."),
                      ("-m", "Every shingle counts once a text: -m %s is not supported (it belongs to `keyphrases extract`)."),
                      ("-u", "Every shingle counts once a text: -u %s is not supported (it belongs to `keyphrases extract`)."),
                      ("-z", "Shingle overlap scores no keyphrases: -z %s is not supported.")):
        if key in opts:
            return refuse(line % opts[key] if "%s" in line else line)
    try:
        words = int(opts.get("-x", "4"))
    except ValueError:
        words = 0
    if not 1 <= words <= applications.OVERLAP_MAX_WORDS:
        return refuse("Invalid number of words: '%s'. Please use an integer from 1 to %d." % (opts["-x"], applications.OVERLAP_MAX_WORDS))
    orientation = opts.get("-o", "symmetric").lower()
    if orientation not in ("symmetric", "directed"):
        return refuse("Invalid orientation: '%s'. Please use one of: 'symmetric', 'directed'." % opts["-o"])
    clusters = "-j" in opts
    if clusters:
        if orientation == "directed":
            return refuse("Clusters need a symmetric matrix: -o %s is not supported with -j." % opts["-o"])
        if "-n" in opts:
            return refuse("Clusters are not ranked: -n %s is not supported with -j (use -k for their number)." % opts["-n"])
        threshold, k, fmt, refusal = _clusters_options(opts)
        if refusal:
            return refuse(refusal)
    else:
        if "-k" in opts:
            return refuse("A number of clusters belongs to clusters: -k %s needs a linkage (-j)." % opts["-k"])
        n, _, threshold, refusal = _top_options(opts)
        if refusal:
            return refuse(refusal.replace("relevance threshold", "overlap threshold"))
        fmt = opts.get("-f", "xml").lower()
        if fmt not in ("xml", "csv"):
            return refuse("Unknown overlap format: '%s'. Please use one of: 'xml', 'csv'." % opts["-f"])
    if world > 1:
        return refuse("Shingle overlap runs on one device: a launcher with WORLD_SIZE=%d is not supported." % world)
    if os.environ.get("EAST_HIP_FORCE_DIST") == "1":
        return refuse("Shingle overlap runs on one device: the collective path is not supported.")
    devices = opts.get("-g", os.environ.get("EAST_HIP_DEVICES", "1"))
    try:
        n_ranks = int(devices)
    except ValueError:
        return refuse("Invalid number of GPUs: '%s'." % devices)
    if n_ranks > 1:
        return refuse("Shingle overlap runs on one device: -g %d is not supported." % n_ranks)
    language = opts.get("-l", consts.Language.ENGLISH)
    try:
        measure = relevance.CosineRelevanceMeasure(consts.VectorSpace.WORDS)
        if measure.stopwords_source == "none":
            sys.stderr.write("nltk's English stopword list is not available: no stopwords are removed.\n")
        texts = _read_texts(args[2])
        if clusters:
            found = applications.texts_overlap_clusters(texts, words, threshold, k, opts["-j"], measure, language)
            print(formatting.format_clusters(found, fmt))
        else:
            found = applications.texts_overlap(texts, n, words, orientation, threshold, measure, language)
            print(formatting.format_similar(found, "text", fmt))
    except (exceptions.EastException, applications.RefusedSimilarity) as e:     # (no device, a failed build ...): a message, not a traceback
        print(e)
        return 1
    except Exception as e:                      # (an unknown format)
        print(e)
        return 1
    return 0


def _texts_terms_main(opts, args, world, refuse):
    """`east texts terms <texts>`: the characteristic terms of every text, or with -r / -k of every cluster.  Everything that
    cannot be done is refused with one line (refuse) before a file is read or a measure is made."""
    if len(args) < 3:
        return refuse('Invalid syntax. For text analysis, EAST should be called as:\n\n'
                      '    east [options] texts terms "path/to/texts/dir"')
    numbers = {}
    for key, default, most, what in (("-n", "10", applications.TOP_MAX_N, "number of terms"), ("-u", "1", 2 ** 31 - 1, "number of texts")):
        try:
            numbers[key] = int(opts.get(key, default))
        except ValueError:
            numbers[key] = 0
        if not 1 <= numbers[key] <= most:
            return refuse("Invalid %s: '%s'. Please use an integer %s." % (
                what, opts[key], "from 1 to %d" % most if key == "-n" else "of at least 1"))
    fmt = opts.get("-f", "xml").lower()
    if fmt not in ("xml", "csv"):
        return refuse("Unknown terms format: '%s'. Please use one of: 'xml', 'csv'." % opts["-f"])
    if "-r" in opts and "-k" in opts:
        return refuse("Clusters are cut by a threshold (-r) or by their number (-k): please give one of the two.")
    if "-j" in opts and "-r" not in opts and "-k" not in opts:
        return refuse("A linkage belongs to clusters: -j %s needs a threshold (-r) or a number of clusters (-k)." % opts["-j"])
    threshold = k = None
    if "-r" in opts:
        try:
            threshold = float(opts["-r"])
        except ValueError:
            threshold = float("nan")
        if threshold != threshold:
            return refuse("Invalid similarity threshold: '%s'." % opts["-r"])
    if "-k" in opts:
        try:
            k = int(opts["-k"])
        except ValueError:
            k = 0
        if k < 1:
            return refuse("Invalid number of clusters: '%s'. Please use an integer of at least 1." % opts["-k"])
    if opts.get("-s", consts.RelevanceMeasure.COSINE).lower() != consts.RelevanceMeasure.COSINE:
        return refuse("Characteristic terms are read off the cosine measure's term index: -s %s is not supported." % opts["-s"])
    if opts.get("-v", consts.VectorSpace.STEMS).lower() == consts.VectorSpace.LEMMATA:
        return refuse("Characteristic terms have no lemmatizer: -v %s is not supported (use 'stems' or 'words')." % opts["-v"])
    for key, line in (("-y", "Characteristic terms take no synonyms: -y is not supported."),
                      ("-o", "Characteristic terms have no orientation: -o %s is not supported."),
                      ("-b", "Characteristic terms are listed per text or per cluster of texts: -b %s is not supported."),
                      ("-c", "Characteristic terms build no graph: -c %s is not supported."),
                      ("-p", "Characteristic terms build no graph: -p %s is not supported.")):
        if key in opts:
            return refuse(line % opts[key] if "%s" in line else line)
    if world > 1:
        return refuse("Characteristic terms run on one device: a launcher with WORLD_SIZE=%d is not supported." % world)
    if os.environ.get("EAST_HIP_FORCE_DIST") == "1":
        return refuse("Characteristic terms run on one device: the collective path is not supported.")
    devices = opts.get("-g", os.environ.get("EAST_HIP_DEVICES", "1"))
    try:
        n_ranks = int(devices)
    except ValueError:
        return refuse("Invalid number of GPUs: '%s'." % devices)
    if n_ranks > 1:
        return refuse("Characteristic terms run on one device: -g %d is not supported." % n_ranks)
    linkage = {"linkage": opts["-j"]} if "-j" in opts else {}      # (checked in main, before anything else)
    try:
        measure = relevance.CosineRelevanceMeasure(opts.get("-v", consts.VectorSpace.STEMS), opts.get("-w", consts.TermWeighting.TF_IDF))
        if measure.stopwords_source == "none":
            sys.stderr.write("nltk's English stopword list is not available: no stopwords are removed.\n")
        texts = _read_texts(args[2])
        found = applications.texts_terms(texts, numbers["-n"], numbers["-u"], measure, opts.get("-l", consts.Language.ENGLISH),
                                         threshold, k, **linkage)
        print(formatting.format_terms(found, fmt))
    except (exceptions.EastException, applications.RefusedSimilarity) as e:     # (a missing stemmer, no device, a failed build ...): a message, not a traceback
        print(e)
        return 1
    return 0


def _texts_passages_main(opts, args, world, refuse):
    """`east texts passages <texts>`: the passages every text shares with the -n texts `texts overlap` ranks for it.
    Everything that cannot be done is refused with one line (refuse) before a file is read or a measure is made."""
    if len(args) < 3:
        return refuse('Invalid syntax. For text analysis, EAST should be called as:\n\n'
                      '    east [options] texts passages "path/to/texts/dir"')
    for key, line in (("-s", "Shared passages compare wording, not a relevance measure: -s %s is not supported."),
                      ("-w", "Shared passages weigh no terms: -w %s is not supported."),
                      ("-v", "Passages are made of words: -v %s is not supported."),
                      ("-y", "Shared passages take no synonyms: -y is not supported."),
                      ("-b", "Shared passages compare texts: -b %s is not supported."),
                      ("-c", "Shared passages build no graph: -c %s is not supported."),
                      ("-p", "Shared passages build no graph: -p %s is not supported."),
                      ("-u", "Shared passages count no texts: -u %s is not supported (it belongs to `keyphrases extract`)."),
                      ("-z", "Shared passages score no keyphrases: -z %s is not supported.")):
        if key in opts:
            return refuse(line % opts[key] if "%s" in line else line)
    numbers = {}
    for key, default, least, most, what in (("-x", "4", 1, applications.OVERLAP_MAX_WORDS, "number of words"),
                                            ("-m", None, None, None, "least number of words of a passage"),
                                            ("-k", "5", 0, None, "number of passages per pair")):
        if key == "-m":
            default, least = str(numbers["-x"]), numbers["-x"]
        try:
            numbers[key] = int(opts.get(key, default))
        except ValueError:
            numbers[key] = least - 1
        if numbers[key] < least or (most is not None and numbers[key] > most):
            bounds = "from %d to %d" % (least, most) if most is not None else "of at least %d" % least
            return refuse("Invalid %s: '%s'. Please use an integer %s." % (what, opts[key], bounds))
    orientation = opts.get("-o", "symmetric").lower()
    if orientation not in ("symmetric", "directed"):
        return refuse("Invalid orientation: '%s'. Please use one of: 'symmetric', 'directed'." % opts["-o"])
    n, _, threshold, refusal = _top_options(opts)
    if refusal:
        return refuse(refusal.replace("relevance threshold", "overlap threshold"))
    fmt = opts.get("-f", "xml").lower()
    if fmt not in ("xml", "csv"):
        return refuse("Unknown passages format: '%s'. Please use one of: 'xml', 'csv'." % opts["-f"])
    if world > 1:
        return refuse("Shared passages run on one device: a launcher with WORLD_SIZE=%d is not supported." % world)
    if os.environ.get("EAST_HIP_FORCE_DIST") == "1":
        return refuse("Shared passages run on one device: the collective path is not supported.")
    devices = opts.get("-g", os.environ.get("EAST_HIP_DEVICES", "1"))
    try:
        n_ranks = int(devices)
    except ValueError:
        return refuse("Invalid number of GPUs: '%s'." % devices)
    if n_ranks > 1:
        return refuse("Shared passages run on one device: -g %d is not supported." % n_ranks)
    language = opts.get("-l", consts.Language.ENGLISH)
    try:
        measure = relevance.CosineRelevanceMeasure(consts.VectorSpace.WORDS)
        if measure.stopwords_source == "none":
            sys.stderr.write("nltk's English stopword list is not available: no stopwords are removed.\n")
        texts = _read_texts(args[2])
        found = applications.texts_passages(texts, n, numbers["-x"], numbers["-m"], numbers["-k"], orientation, threshold, None, measure, language)
        print(formatting.format_passages(found, fmt))
    except exceptions.EastException as e:       # (no device, a failed build ...): a message, not a traceback
        print(e)
        return 1
    except Exception as e:                      # (an unknown format)
        print(e)
        return 1
    return 0


def _linkage_refusal(opts, args):
    """The one line that refuses -j, or None: a linkage belongs to `texts clusters` and `keyphrases clusters` -- and to the
    clusters `texts terms` labels -- and is one of applications.LINKAGES."""
    if "-j" not in opts:
        return None
    if args[:2] not in (["texts", "clusters"], ["keyphrases", "clusters"], ["texts", "terms"], ["texts", "overlap"]):
        return "A linkage belongs to clusters: -j %s is supported by `texts clusters` and `keyphrases clusters` only." % opts["-j"]
    if opts["-j"] not in applications.LINKAGES:
        return "Unknown linkage: '%s'. Please use one of: 'single', 'complete', 'average'." % opts["-j"]
    return None


def _clusters_options(opts):
    """(threshold, k, format, None) of `texts clusters` and `keyphrases clusters`, or (None, None, None, the one line that
    says what is wrong)."""
    fmt = opts.get("-f", "xml").lower()
    if fmt not in ("xml", "csv", "merges"):
        return None, None, None, "Unknown clusters format: '%s'. Please use one of: 'xml', 'csv', 'merges'." % opts["-f"]
    if "-r" in opts and "-k" in opts:
        return None, None, None, "Clusters are cut by a threshold (-r) or by their number (-k): please give one of the two."
    if "-r" not in opts and "-k" not in opts and fmt != "merges":
        return None, None, None, "Clusters need a threshold (-r) or their number (-k); without either only -f merges has something to print."
    threshold = k = None
    if "-r" in opts:
        try:
            threshold = float(opts["-r"])
        except ValueError:
            threshold = float("nan")
        if threshold != threshold:
            return None, None, None, "Invalid similarity threshold: '%s'." % opts["-r"]
    if "-k" in opts:
        try:
            k = int(opts["-k"])
        except ValueError:
            k = 0
        if k < 1:
            return None, None, None, "Invalid number of clusters: '%s'. Please use an integer of at least 1." % opts["-k"]
    return threshold, k, fmt, None


def _clusters_main(opts, args, world, rank):
    """`east texts clusters <texts>` and `east keyphrases clusters <keyphrases file> <texts>`.  Everything that cannot be done
    is refused with one line before a file is read or anything touches a device."""
    def refuse(line):
        if rank == 0:
            print(line)
        return 1

    of_texts = args[0] == "texts"
    if len(args) < (3 if of_texts else 4):
        return refuse('Invalid syntax. For clusters, EAST should be called as:\n\n'
                      '    east [options] texts clusters "path/to/texts/dir"\n'
                      '    east [options] keyphrases clusters "path/to/keyphrases.txt" "path/to/texts/dir"')
    threshold, k, fmt, refusal = _clusters_options(opts)
    if refusal:
        return refuse(refusal)
    measure_name = opts.get("-s", consts.RelevanceMeasure.AST).lower()
    cosine = measure_name == consts.RelevanceMeasure.COSINE
    bm25 = measure_name == consts.RelevanceMeasure.BM25      # (keyphrases clusters: `texts clusters` was refused in main)
    if measure_name != consts.RelevanceMeasure.AST.lower() and not cosine and not bm25:
        return refuse("Relevance measure '%s' is not available (use 'ast', 'cosine' or 'bm25')." % opts["-s"])
    by = opts.get("-b", "text").lower()
    if by not in ("text", "keyphrase"):
        return refuse("Invalid clustering direction: '%s'. Please use one of: 'text', 'keyphrase'." % opts["-b"])
    if of_texts and "-b" in opts:
        return refuse("`texts clusters` groups the texts: -b %s is not supported (a direction belongs to `keyphrases clusters`)." % opts["-b"])
    if "-o" in opts:
        return refuse("Clusters need a symmetric matrix: -o %s is not supported." % opts["-o"])
    if "-n" in opts:
        return refuse("Clusters are not ranked: -n %s is not supported (use -k for their number)." % opts["-n"])
    if "-y" in opts:
        return refuse("Clusters take no synonyms: -y is not supported.")
    if opts.get("-v", consts.VectorSpace.STEMS).lower() == consts.VectorSpace.LEMMATA:
        return refuse("Clusters have no lemmatizer: -v %s is not supported (use 'stems' or 'words')." % opts["-v"])
    if world > 1:
        return refuse("Clusters run on one device: a launcher with WORLD_SIZE=%d is not supported." % world)
    if os.environ.get("EAST_HIP_FORCE_DIST") == "1":
        return refuse("Clusters run on one device: the collective path is not supported.")
    devices = opts.get("-g", os.environ.get("EAST_HIP_DEVICES", "1"))
    try:
        n_ranks = int(devices)
    except ValueError:
        return refuse("Invalid number of GPUs: '%s'." % devices)
    if n_ranks > 1:
        return refuse("Clusters run on one device: -g %d is not supported." % n_ranks)
    language = opts.get("-l", consts.Language.ENGLISH)
    linkage = {"linkage": opts["-j"]} if "-j" in opts else {}      # (checked in main, before anything else)
    try:
        if cosine or bm25:
            if bm25:
                measure = relevance.BM25RelevanceMeasure(opts.get("-v", consts.VectorSpace.STEMS), *_bm25_parameters(opts))
            else:
                measure = relevance.CosineRelevanceMeasure(opts.get("-v", consts.VectorSpace.STEMS), opts.get("-w", consts.TermWeighting.TF_IDF))
            if measure.stopwords_source == "none":
                sys.stderr.write("nltk's English stopword list is not available: no stopwords are removed.\n")
        else:
            measure = relevance.ASTRelevanceMeasure(opts.get("-a", consts.ASTAlgorithm.EASA), "-d" not in opts)
        if of_texts:
            found = applications.texts_clusters(_read_texts(args[2]), threshold, k, measure, language, **linkage)
        else:
            keyphrases = _read(os.path.abspath(args[2])).decode("utf-8", errors="replace").splitlines()
            found = applications.keyphrases_clusters(keyphrases, _read_texts(args[3]), by, threshold, k, measure, None, language,
                                                     **linkage)
        print(formatting.format_clusters(found, fmt))
    except (exceptions.EastException, applications.RefusedSimilarity) as e:     # (a missing stemmer, no device, a failed build ...): a message, not a traceback
        print(e)
        return 1
    return 0


def _extract_options(opts):
    """(n, max_words, min_count, min_texts, format, None) of `keyphrases extract`, or five times None and the one line that
    says what is wrong."""
    numbers = []
    for key, default, least, most, what in (("-n", "100", 0, None, "number of phrases"), ("-x", "3", 1, applications.EXTRACT_MAX_WORDS, "number of words"),
                                            ("-m", "2", 1, None, "number of occurrences"), ("-u", "1", 1, None, "number of texts")):
        try:
            value = int(opts.get(key, default))
        except ValueError:
            value = None
        if value is None or value < least or (most is not None and value > most) or value >= 2 ** 31:
            return (None,) * 5 + ("Invalid %s: '%s'. Please use an integer %s." % (
                what, opts[key], "from %d to %d" % (least, most) if most is not None else "of at least %d" % least),)
        numbers.append(value)
    fmt = opts.get("-f", "txt").lower()
    if fmt not in ("txt", "csv", "xml"):
        return (None,) * 5 + ("Unknown phrases format: '%s'. Please use one of: 'txt', 'csv', 'xml'." % opts["-f"],)
    return tuple(numbers) + (fmt, None)


def _extract_main(opts, args, world, rank):
    """`east keyphrases extract <texts>`.  Everything that cannot be done is refused with one line before a file is read or
    anything touches a device."""
    def refuse(line):
        if rank == 0:
            print(line)
        return 1

    if len(args) < 3:
        return refuse('Invalid syntax. For phrase extraction, EAST should be called as:\n\n'
                      '    east [options] keyphrases extract "path/to/texts/dir"')
    n, max_words, min_count, min_texts, fmt, refusal = _extract_options(opts)
    if refusal:
        return refuse(refusal)
    if "-s" in opts:
        return refuse("Phrases are counted, not scored: -s %s is not supported (score the extracted phrases with `keyphrases table` or `top`)." % opts["-s"])
    if "-w" in opts:
        return refuse("Phrases are counted, not weighted: -w %s is not supported." % opts["-w"])
    if opts.get("-v", consts.VectorSpace.WORDS).lower() != consts.VectorSpace.WORDS:
        return refuse("Phrases are made of words: -v %s is not supported." % opts["-v"])
    for key, line in (("-y", "Phrase extraction takes no synonyms: -y is not supported."),
                      ("-o", "Phrases have no orientation: -o %s is not supported."),
                      ("-b", "Phrases are extracted from the whole collection: -b %s is not supported."),
                      ("-r", "Phrases have no relevance threshold: -r %s is not supported (use -m for occurrences, -u for texts)."),
                      ("-k", "Phrases are not clustered: -k %s is not supported (use -n for their number)."),
                      ("-c", "Phrase extraction builds no graph: -c %s is not supported."),
                      ("-p", "Phrase extraction builds no graph: -p %s is not supported.")):
        if key in opts:
            return refuse(line % opts[key] if "%s" in line else line)
    if world > 1:
        return refuse("Phrase extraction runs on one device: a launcher with WORLD_SIZE=%d is not supported." % world)
    if os.environ.get("EAST_HIP_FORCE_DIST") == "1":
        return refuse("Phrase extraction runs on one device: the collective path is not supported.")
    devices = opts.get("-g", os.environ.get("EAST_HIP_DEVICES", "1"))
    try:
        n_ranks = int(devices)
    except ValueError:
        return refuse("Invalid number of GPUs: '%s'." % devices)
    if n_ranks > 1:
        return refuse("Phrase extraction runs on one device: -g %d is not supported." % n_ranks)
    try:
        measure = relevance.CosineRelevanceMeasure(consts.VectorSpace.WORDS)
        if measure.stopwords_source == "none":
            sys.stderr.write("nltk's English stopword list is not available: no stopwords are removed.\n")
        texts = _read_texts(args[2])
        found = applications.keyphrases_extract(texts, n, max_words, 1, min_count, min_texts, measure,
                                                opts.get("-l", consts.Language.ENGLISH))
        sys.stdout.write(formatting.format_phrases(found, fmt))       # (txt: a keyphrase file, no line added)
    except exceptions.EastException as e:       # (no device, a failed build ...): a message, not a traceback
        print(e)
        return 1
    return 0


def _run_cosine(subcommand, keyphrases, texts, opts, synonimizer=None):
    """-s cosine with its -w / -v options (reference main.py:95-98, relevance.py:58-62); bad values, -v lemmata and a
    missing stemmer end here with one line, before anything touches the device."""
    try:
        measure = relevance.CosineRelevanceMeasure(opts.get("-v", consts.VectorSpace.STEMS),
                                                   opts.get("-w", consts.TermWeighting.TF_IDF))
        if measure.stopwords_source == "none":
            sys.stderr.write("nltk's English stopword list is not available: no stopwords are removed.\n")
        return _run(subcommand, keyphrases, texts, measure, opts, synonimizer)
    except exceptions.EastException as e:
        print(e)
        return 1


def _bm25_parameters(opts):
    """(k1, b) of -z k1,b (default 1.2,0.75); ValueError for anything else than two numbers with k1 finite and >= 0 and
    0 <= b <= 1."""
    if "-z" not in opts:
        return relevance.BM25_K1, relevance.BM25_B
    parts = opts["-z"].split(",")
    if len(parts) != 2:
        raise ValueError("two numbers")
    return relevance.bm25_parameters(float(parts[0]), float(parts[1]))


def _bm25_refusal(opts, args, world):
    """The one line that says why a command line with `-s bm25` or `-z` cannot run, or None.  Nothing is read and no device
    is touched."""
    bm25 = opts.get("-s", "").lower() == consts.RelevanceMeasure.BM25
    if "-z" in opts and not bm25:
        return "Option -z gives the k1,b of the BM25 measure: use it with -s bm25."
    if not bm25:
        return None
    if args[:1] == ["texts"] or args[:2] == ["keyphrases", "extract"]:
        return ("Relevance measure 'bm25' scores keyphrases against texts: `%s` is not supported (the texts alone are the "
                "cosine measure's: -s cosine)." % " ".join(args[:2]))
    if "-w" in opts:
        return "Relevance measure 'bm25' has no term weighting: -w %s is not supported (it belongs to -s cosine; see -z k1,b)." % opts["-w"]
    try:
        _bm25_parameters(opts)
    except ValueError:
        return "Invalid BM25 parameters: '%s'. Please use -z k1,b with k1 >= 0 and 0 <= b <= 1 (default 1.2,0.75)." % opts["-z"]
    if opts.get("-v", consts.VectorSpace.STEMS).lower() == consts.VectorSpace.LEMMATA:
        return "Relevance measure 'bm25' has no lemmatizer: -v %s is not supported (use 'stems' or 'words')." % opts["-v"]
    if world > 1:
        return "Relevance measure 'bm25' runs on one device: a launcher with WORLD_SIZE=%d is not supported." % world
    if os.environ.get("EAST_HIP_FORCE_DIST") == "1":
        return "Relevance measure 'bm25' runs on one device: the collective path is not supported."
    devices = opts.get("-g", os.environ.get("EAST_HIP_DEVICES", "1"))
    try:
        n_ranks = int(devices)
    except ValueError:
        return "Invalid number of GPUs: '%s'." % devices
    if n_ranks > 1:
        return "Relevance measure 'bm25' runs on one device: -g %d is not supported." % n_ranks
    return None


def _run_bm25(subcommand, keyphrases, texts, opts, synonimizer=None):
    """-s bm25 with its -v / -z options; what _bm25_refusal lets through and the measure still refuses (an unknown -v, a
    missing stemmer) ends here with one line, before anything touches the device."""
    try:
        measure = relevance.BM25RelevanceMeasure(opts.get("-v", consts.VectorSpace.STEMS), *_bm25_parameters(opts))
        if measure.stopwords_source == "none":
            sys.stderr.write("nltk's English stopword list is not available: no stopwords are removed.\n")
        return _run(subcommand, keyphrases, texts, measure, opts, synonimizer)
    except exceptions.EastException as e:
        print(e)
        return 1


def _top_options(opts):
    """(n, by, threshold, None) of `keyphrases top` and `keyphrases similar`, or (None, None, None, the one line that says what is wrong)."""
    try:
        n = int(opts.get("-n", "10"))
    except ValueError:
        return None, None, None, "Invalid number of entries: '%s'. Please use an integer from 1 to %d." % (
            opts["-n"], applications.TOP_MAX_N)
    if not 1 <= n <= applications.TOP_MAX_N:
        return None, None, None, "Invalid number of entries: '%s'. Please use an integer from 1 to %d." % (
            opts["-n"], applications.TOP_MAX_N)
    by = opts.get("-b", "text").lower()
    if by not in ("text", "keyphrase"):
        return None, None, None, "Invalid ranking direction: '%s'. Please use one of: 'text', 'keyphrase'." % opts["-b"]
    threshold = None
    if "-r" in opts:
        try:
            threshold = float(opts["-r"])
        except ValueError:
            threshold = float("nan")
        if threshold != threshold:
            return None, None, None, "Invalid relevance threshold: '%s'." % opts["-r"]
    return n, by, threshold, None


def _run(subcommand, keyphrases, texts, similarity_measure, opts, synonimizer=None):
    if subcommand == "table":
        table = applications.keyphrases_table(keyphrases, texts, similarity_measure, synonimizer, opts["-l"])
        table_format = opts.get("-f", "xml").lower()
        try:
            print(formatting.format_table(table, table_format))
        except Exception as e:
            print(e)
            return 1
        return 0
    elif subcommand == "graph":                                                                 # main.py:124-143
        opts.setdefault("-c", "0.6")    # referral confidence
        opts.setdefault("-r", "0.25")   # relevance threshold of the matching score
        opts.setdefault("-p", "1")      # support threshold for graph nodes
        # (the graph as arrays: the formatters write it from them, no dict per edge)
        graph = applications.keyphrases_graph_arrays(keyphrases, texts, float(opts["-c"]), float(opts["-r"]),
                                                     float(opts["-p"]), similarity_measure, synonimizer, opts["-l"])
        graph_format = opts.get("-f", "edges").lower()
        try:
            print(formatting.format_graph(graph, graph_format))
        except Exception as e:
            print(e)
            return 1
        return 0
    elif subcommand == "top":
        n, by, threshold, _ = _top_options(opts)
        top = applications.keyphrases_top(keyphrases, texts, n, by, threshold, similarity_measure, synonimizer, opts["-l"])
        try:
            print(formatting.format_top(top, by, opts.get("-f", "xml").lower()))
        except Exception as e:
            print(e)
            return 1
        return 0
    elif subcommand == "similar":
        n, by, threshold, _ = _top_options(opts)
        similar = applications.keyphrases_similar(keyphrases, texts, n, by, threshold, similarity_measure, synonimizer, opts["-l"])
        try:
            print(formatting.format_similar(similar, by, opts.get("-f", "xml").lower()))
        except Exception as e:
            print(e)
            return 1
        return 0
    print("Invalid subcommand: '%s'. Please use one of: 'table', 'graph', 'top', 'similar', 'clusters', 'extract'." % subcommand)
    return 1


if __name__ == "__main__":
    sys.exit(main())
