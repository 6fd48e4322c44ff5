# -*- coding: utf-8 -*-
"""Text renderings of the keyphrase table and the keyphrase graph.

Byte-for-byte the outputs of the reference's east/formatting.py (table2xml, table2csv,
graph2gml, graph2edges) -- pinned by fixtures generated from it -- with two documented fixes:
format_table works (the reference refers to an undefined name) and graph2edges looks nodes up
by id (the reference indexes the node list, which breaks once a node was filtered out).
"""

_SCORE = "%.3f"


def format_table(table, format):
    renderers = {"xml": table2xml, "csv": table2csv}
    if format not in renderers:
        raise Exception("Unknown table format: '%s'. Please use one of: 'xml', 'csv'." % format)
    return renderers[format](table)


def _bulk(keyphrases_table, kind):
    """A ScoreTable (applications.py) of many scores goes through the library's host-side formatter -- the same bytes,
    written by a few threads straight from the score array -- instead of one Python '%.3f' per score.  None: not such a
    table (a plain dict, a small table, names or scores the formatter does not take)."""
    from east import applications
    if not isinstance(keyphrases_table, applications.ScoreTable) or keyphrases_table.scores.size < _BULK_MIN_SCORES:
        return None
    import numpy as np
    table = keyphrases_table
    scores = np.asarray(table.scores, dtype=np.float64)
    titles = table.text_titles
    if len(table) == 0 or len(set(titles)) != len(titles) or not np.isfinite(scores).all() or np.abs(scores).max() >= 1e15:
        return None
    try:
        from east import hip_backend
        kp_order = sorted(range(len(table.keyphrases)), key=table.keyphrases.__getitem__)
        text_order = sorted(range(len(titles)), key=titles.__getitem__)
        if kind == "xml":
            return hip_backend.format_table(scores, kp_order, text_order, table.keyphrases, titles, "xml")
        return hip_backend.format_table(scores, kp_order, text_order, [_csv_quote(k) for k in table.keyphrases],
                                        [_csv_quote(t) for t in titles], "csv")
    except (ValueError, UnicodeError, Exception) as e:       # noqa: BLE001 (the library is missing, a NUL in a name ...)
        from east import exceptions
        if isinstance(e, (ValueError, UnicodeError, exceptions.HipBackendError)):
            return None
        raise


_BULK_MIN_SCORES = 4096


def table2xml(keyphrases_table):
    """<table> / <keyphrase value=..> / <text name=..>score</text>, keyphrases and texts sorted."""
    text = _bulk(keyphrases_table, "xml")
    if text is not None:
        return text
    lines = ["<table>"]
    for keyphrase in sorted(keyphrases_table):
        row = keyphrases_table[keyphrase]
        lines.append('  <keyphrase value="%s">' % keyphrase)
        lines.extend('    <text name="%s">%s</text>' % (text, _SCORE % row[text]) for text in sorted(row))
        lines.append("  </keyphrase>")
    lines.append("</table>")
    return "\n".join(lines) + "\n"


def _csv_quote(value):
    return '"%s"' % value.replace('"', "'")


def table2csv(keyphrases_table):
    """Header row of quoted keyphrases, then one row per text: "name",score,score,..."""
    text = _bulk(keyphrases_table, "csv")
    if text is not None:
        return text
    keyphrases = sorted(keyphrases_table)
    texts = sorted(keyphrases_table[keyphrases[0]])
    rows = ["," + ",".join(_csv_quote(k) for k in keyphrases)]
    for text in texts:
        scores = [_SCORE % keyphrases_table[k][text] for k in keyphrases]
        rows.append(",".join([_csv_quote(text)] + scores))
    return "\n".join(rows) + "\n"


def format_top(top, by, format):
    """A ranking (applications.keyphrases_top: {segment: [(member, score), ...]}, by = "text" or "keyphrase")."""
    renderers = {"xml": top2xml, "csv": top2csv}
    if format not in renderers:
        raise Exception("Unknown ranking format: '%s'. Please use one of: 'xml', 'csv'." % format)
    if by not in ("text", "keyphrase"):
        raise Exception("Unknown ranking direction: '%s'. Please use one of: 'text', 'keyphrase'." % by)
    return renderers[format](top, by)


def top2xml(top, by):
    """<top by=..> / <text name=..> / <keyphrase value=.. rank=..>score</keyphrase> (the two roles swapped for
    by="keyphrase"); segments sorted by name as table2xml sorts, entries in rank order."""
    outer, inner = (("text", "name"), ("keyphrase", "value")) if by == "text" else (("keyphrase", "value"), ("text", "name"))
    lines = ['<top by="%s">' % by]
    for segment in sorted(top):
        lines.append('  <%s %s="%s">' % (outer[0], outer[1], segment))
        lines.extend('    <%s %s="%s" rank="%d">%s</%s>' % (inner[0], inner[1], member, rank, _SCORE % score, inner[0])
                     for rank, (member, score) in enumerate(top[segment], 1))
        lines.append("  </%s>" % outer[0])
    lines.append("</top>")
    return "\n".join(lines) + "\n"


def top2csv(top, by):
    """One line per entry: "segment","member",rank,score; segments sorted by name, entries in rank order."""
    return "".join("%s,%s,%d,%s\n" % (_csv_quote(segment), _csv_quote(member), rank, _SCORE % score)
                   for segment in sorted(top) for rank, (member, score) in enumerate(top[segment], 1))


def format_similar(result, by, format):
    """Similar members (applications.keyphrases_similar: {member: [(other member, similarity), ...]}, by = "text" or
    "keyphrase")."""
    renderers = {"xml": similar2xml, "csv": similar2csv}
    if format not in renderers:
        raise Exception("Unknown similarity format: '%s'. Please use one of: 'xml', 'csv'." % format)
    if by not in ("text", "keyphrase"):
        raise Exception("Unknown similarity direction: '%s'. Please use one of: 'text', 'keyphrase'." % by)
    return renderers[format](result, by)


def similar2xml(result, by):
    """<similar by=..> / <text name=..> / <text name=.. rank=..>similarity</text> (<keyphrase value=..> on both levels for
    by="keyphrase"); members sorted by name as top2xml sorts, entries in rank order."""
    element, attribute = ("text", "name") if by == "text" else ("keyphrase", "value")
    lines = ['<similar by="%s">' % by]
    for member in sorted(result):
        lines.append('  <%s %s="%s">' % (element, attribute, member))
        lines.extend('    <%s %s="%s" rank="%d">%s</%s>' % (element, attribute, other, rank, _SCORE % similarity, element)
                     for rank, (other, similarity) in enumerate(result[member], 1))
        lines.append("  </%s>" % element)
    lines.append("</similar>")
    return "\n".join(lines) + "\n"


def similar2csv(result, by):
    """One line per entry: "member","other",rank,similarity; members sorted by name, entries in rank order."""
    return "".join("%s,%s,%d,%s\n" % (_csv_quote(member), _csv_quote(other), rank, _SCORE % similarity)
                   for member in sorted(result) for rank, (other, similarity) in enumerate(result[member], 1))


def format_related(result, format):
    """Related texts (applications.texts_related: {text: [(other text, relatedness), ...]}), in the layout of
    format_similar(..., "text", ...) under the root element <related>."""
    renderers = {"xml": related2xml, "csv": related2csv}
    if format not in renderers:
        raise Exception("Unknown relatedness format: '%s'. Please use one of: 'xml', 'csv'." % format)
    return renderers[format](result)


def related2xml(result):
    """<related> / <text name=..> / <text name=.. rank=..>relatedness</text>; texts sorted by name, entries in rank order."""
    lines = ["<related>"]
    for text in sorted(result):
        lines.append('  <text name="%s">' % text)
        lines.extend('    <text name="%s" rank="%d">%s</text>' % (other, rank, _SCORE % value)
                     for rank, (other, value) in enumerate(result[text], 1))
        lines.append("  </text>")
    lines.append("</related>")
    return "\n".join(lines) + "\n"


def related2csv(result):
    """One line per entry: "text","other",rank,relatedness; texts sorted by name, entries in rank order."""
    return similar2csv(result, "text")


def format_clusters(clustering, format):
    """Clusters (applications.Clustering).  xml and csv list the flat clusters and need a cut (a threshold or k); merges
    lists the dendrogram and needs none."""
    renderers = {"xml": clusters2xml, "csv": clusters2csv, "merges": clusters2merges}
    if format not in renderers:
        raise Exception("Unknown clusters format: '%s'. Please use one of: 'xml', 'csv', 'merges'." % format)
    if format != "merges" and clustering.clusters is None:
        raise Exception("Clusters format '%s' lists flat clusters: give a threshold or a number of clusters." % format)
    return renderers[format](clustering)


def clusters2xml(clustering):
    """<clusters count=..> / <cluster id=.. size=..> / <member name=../>; the clusters by their smallest member, numbered
    from 1, the members in index order."""
    lines = ['<clusters count="%d">' % len(clustering.clusters)]
    for number, members in enumerate(clustering.clusters, 1):
        lines.append('  <cluster id="%d" size="%d">' % (number, len(members)))
        lines.extend('    <member name="%s"/>' % member for member in members)
        lines.append("  </cluster>")
    lines.append("</clusters>")
    return "\n".join(lines) + "\n"


def clusters2csv(clustering):
    """One line per member: "member",cluster number,"the cluster's first member"; in the order of clusters2xml."""
    return "".join("%s,%d,%s\n" % (_csv_quote(member), number, _csv_quote(members[0]))
                   for number, members in enumerate(clustering.clusters, 1) for member in members)


def clusters2merges(clustering):
    """One line per merge of the dendrogram, strongest first: "member","member",similarity."""
    return "".join("%s,%s,%s\n" % (_csv_quote(a), _csv_quote(b), _SCORE % similarity) for a, b, similarity in clustering.merges)


def format_phrases(result, format="txt"):
    """Extracted phrases (applications.keyphrases_extract: [Phrase(text, words, count, texts, score)], best first).  txt:
    one phrase a line and nothing else -- exactly a keyphrase file."""
    renderers = {"txt": phrases2txt, "csv": phrases2csv, "xml": phrases2xml}
    if format not in renderers:
        raise Exception("Unknown phrases format: '%s'. Please use one of: 'txt', 'csv', 'xml'." % format)
    return renderers[format](result)


def phrases2txt(result):
    return "".join("%s\n" % phrase.text for phrase in result)


def phrases2csv(result):
    """One line per phrase, best first: "phrase",words,count,texts,score."""
    return "".join("%s,%d,%d,%d,%d\n" % (_csv_quote(p.text), p.words, p.count, p.texts, p.score) for p in result)


def phrases2xml(result):
    """<phrases count=..> / <phrase rank=.. words=.. count=.. texts=.. score=..>text</phrase>, best first."""
    lines = ['<phrases count="%d">' % len(result)]
    lines.extend('  <phrase rank="%d" words="%d" count="%d" texts="%d" score="%d">%s</phrase>'
                 % (rank, p.words, p.count, p.texts, p.score, p.text) for rank, p in enumerate(result, 1))
    lines.append("</phrases>")
    return "\n".join(lines) + "\n"


def format_passages(result, format):
    """Shared passages (applications.texts_passages: {text: [PassagePair(other, value, starts, covered, found, [Passage(start,
    words, at, text)])]})."""
    renderers = {"xml": passages2xml, "csv": passages2csv}
    if format not in renderers:
        raise Exception("Unknown passages format: '%s'. Please use one of: 'xml', 'csv'." % format)
    return renderers[format](result)


def _passage_value(value):
    return "" if value is None else _SCORE % value


def passages2xml(result):
    """<passages> / <text name=..> / <text name=.. rank=.. value=.. starts=.. covered=.. found=..> / <passage start=.. words=..
    at=..>text</passage>; texts sorted by name, the others in the order given, the passages longest first.  value is left
    out where the pairs were named, not ranked."""
    lines = ["<passages>"]
    for text in sorted(result):
        lines.append('  <text name="%s">' % text)
        for rank, pair in enumerate(result[text], 1):
            value = "" if pair.value is None else ' value="%s"' % _passage_value(pair.value)
            lines.append('    <text name="%s" rank="%d"%s starts="%d" covered="%d" found="%d">' % (pair.other, rank, value, pair.starts, pair.covered, pair.found))
            lines.extend('      <passage start="%d" words="%d" at="%d">%s</passage>' % (p.start, p.words, p.at, p.text) for p in pair.passages)
            lines.append("    </text>")
        lines.append("  </text>")
    lines.append("</passages>")
    return "\n".join(lines) + "\n"


def passages2csv(result):
    """One line per passage: "text","other",value,start,words,at,"passage"; in the order of passages2xml; value is empty
    where the pairs were named, not ranked."""
    return "".join("%s,%s,%s,%d,%d,%d,%s\n" % (_csv_quote(text), _csv_quote(pair.other), _passage_value(pair.value), p.start, p.words, p.at, _csv_quote(p.text))
                   for text in sorted(result) for pair in result[text] for p in pair.passages)


def format_terms(result, format):
    """Characteristic terms (applications.texts_terms: [TermGroup(names, [Term(text, value, texts, df)])])."""
    renderers = {"xml": terms2xml, "csv": terms2csv}
    if format not in renderers:
        raise Exception("Unknown terms format: '%s'. Please use one of: 'xml', 'csv'." % format)
    return renderers[format](result)


def terms2xml(result):
    """<terms groups=..> / <group id=.. size=..> / <member name=../> ... <term rank=.. texts=.. df=.. value=..>text</term>; the
    groups in the order given, numbered from 1, the terms best first."""
    lines = ['<terms groups="%d">' % len(result)]
    for number, group in enumerate(result, 1):
        lines.append('  <group id="%d" size="%d">' % (number, len(group.names)))
        lines.extend('    <member name="%s"/>' % name for name in group.names)
        lines.extend('    <term rank="%d" texts="%d" df="%d" value="%s">%s</term>' % (rank, t.texts, t.df, _SCORE % t.value, t.text)
                     for rank, t in enumerate(group.terms, 1))
        lines.append("  </group>")
    lines.append("</terms>")
    return "\n".join(lines) + "\n"


def terms2csv(result):
    """One line per (group, term): "the group's members joined by |","term",value,texts,df; groups in the order given, terms best first."""
    return "".join("%s,%s,%s,%d,%d\n" % (_csv_quote("|".join(group.names)), _csv_quote(t.text), _SCORE % t.value, t.texts, t.df)
                   for group in result for t in group.terms)


def format_graph(graph, format):
    renderers = {"gml": graph2gml, "edges": graph2edges}
    if format not in renderers:
        raise Exception("Unknown graph format: '%s'. Please use one of: 'gml', 'edges'." % format)
    return renderers[format](graph)


def _as_arrays(graph):
    """The graph if it is a KeyphraseGraph (applications.py), else None."""
    from east import applications
    return graph if isinstance(graph, applications.KeyphraseGraph) else None


def _edges_from_arrays(graph):
    """graph2edges off the arrays: the edges of a source are one stretch of the edge arrays, so a line is made per stretch
    (a label listed twice gathers its stretches in the line of its first appearance, as the dict form does)."""
    import numpy as np
    labels, source, target = graph.keyphrases, graph.edge_source, graph.edge_target.tolist()
    starts = np.flatnonzero(np.diff(source)) + 1 if len(source) else np.zeros(0, dtype=np.int64)
    bounds = [0] + starts.tolist() + [len(source)]
    targets = {}
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b > a:
            targets.setdefault(labels[int(source[a])], []).extend(map(labels.__getitem__, target[a:b]))
    return "".join("%s -> %s\n" % (label, ", ".join(found)) for label, found in targets.items())


def _gml_from_arrays(graph):
    """graph2gml off the arrays: one format per node and per edge, no dict in between."""
    out = ["graph", "[", "  directed 1",
           "  referral_confidence %.2f" % graph.referral_confidence,
           "  relevance_threshold %.2f" % graph.relevance_threshold,
           "  support_threshold %i" % graph.support_threshold]
    out += ['  node\n  [\n    id %i\n    label "%s"\n  ]' % (position, graph.keyphrases[position])
            for position in graph.node_ids.tolist()]
    out += ["  edge\n  [\n    source %i\n    target %i\n    confidence %.2f\n  ]" % edge
            for edge in zip(graph.edge_source.tolist(), graph.edge_target.tolist(), graph.edge_confidence.tolist())]
    out.append("]")
    return "\n".join(out) + "\n"


def graph2edges(graph):
    """One line per source node: `label -> label, label`, in order of first appearance."""
    if _as_arrays(graph) is not None:
        return _edges_from_arrays(graph)
    label_of = dict((node["id"], node["label"]) for node in graph["nodes"])
    targets = {}
    for edge in graph["edges"]:
        targets.setdefault(label_of[edge["source"]], []).append(label_of[edge["target"]])
    return "".join("%s -> %s\n" % (source, ", ".join(found)) for source, found in targets.items())


def graph2gml(graph):
    """Graph Modelling Language: header with the three thresholds, a node block per node, an edge block per edge."""
    if _as_arrays(graph) is not None:
        return _gml_from_arrays(graph)
    out = ["graph", "[", "  directed 1",
           "  referral_confidence %.2f" % graph["referral_confidence"],
           "  relevance_threshold %.2f" % graph["relevance_threshold"],
           "  support_threshold %i" % graph["support_threshold"]]
    for node in graph["nodes"]:
        out += ["  node", "  [", "    id %i" % node["id"], '    label "%s"' % node["label"], "  ]"]
    for edge in graph["edges"]:
        out += ["  edge", "  [", "    source %i" % edge["source"], "    target %i" % edge["target"],
                "    confidence %.2f" % edge["confidence"], "  ]"]
    out.append("]")
    return "\n".join(out) + "\n"
