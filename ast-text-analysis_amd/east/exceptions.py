# -*- coding: utf-8 -*-
"""Exceptions of the EAST surface (reference east/exceptions.py:6-64)."""


class EastException(Exception):
    """Base EAST exception: `msg_fmt` is %-formatted with the constructor kwargs."""
    msg_fmt = "An unknown exception occurred."

    def __init__(self, message=None, **kwargs):
        self.kwargs = kwargs
        if not message:
            try:
                message = self.msg_fmt % kwargs
            except KeyError:
                message = self.msg_fmt
        super(EastException, self).__init__(message)

    def format_message(self):
        return str(self)


class NotFoundException(EastException):
    msg_fmt = "Not found."


class NoSuchASTAlgorithm(NotFoundException):
    msg_fmt = "There is no AST construction algorithm with name `%(name)s`."


class EmptyStringsCollectionException(EastException):
    msg_fmt = "The input strings collection is empty."


class SymbolOutOfDomainException(EastException):
    """New: the reference's string terminators are the code points U+0A00+i (east/asts/utils.py:25-40), so
    its own symbol encoding cannot hold text at or above U+0A00.  Raised where that encoding is asked for
    explicitly (asts/utils.py: strings_to_symbols(tagged=False)); the HIP backend itself indexes such text
    in the tagged encoding."""
    msg_fmt = ("Text%(where)s contains the code point U+%(code)04X, which collides with the "
               "string terminators of the annotated suffix tree (outside the method's domain).")

    def __init__(self, code, document=None):
        """document: index (or name) of the first text the character was found in, if known."""
        self.code, self.document = code, document
        super(SymbolOutOfDomainException, self).__init__(
            code=code, where="" if document is None else " %s" % (repr(document) if isinstance(document, str) else "number %d" % document))


class HipBackendError(EastException):
    """New: the MI355X backend is unavailable or failed.  There is no CPU fallback."""
    msg_fmt = "HIP backend error: %(reason)s"


class NoSuchVectorSpace(NotFoundException):
    """New: -v / CosineRelevanceMeasure(vector_space=...) is none of consts.VectorSpace."""
    msg_fmt = "There is no vector space with name `%(name)s` (use 'words' or 'stems')."


class NoSuchTermWeighting(NotFoundException):
    """New: -w / CosineRelevanceMeasure(term_weighting=...) is none of consts.TermWeighting."""
    msg_fmt = "There is no term weighting with name `%(name)s` (use 'tf' or 'tf-idf')."


class TomitaNotInstalledException(EastException):
    """The reference's name (exceptions.py:57): here it says that no dependency triples were given -- the parser that
    makes them from text is not part of this project."""
    msg_fmt = ("Synonym extraction needs dependency triples: pass `triples=` (Tomita's XML output, or lines of "
               "w1<TAB>relation<TAB>w2); the Tomita parser itself is not available here.")


class TriplesFormatException(EastException):
    """New: a dependency triple that cannot be read (east/synonyms)."""
    msg_fmt = "Malformed dependency triple at line %(line)d of %(source)s: expected w1<TAB>relation<TAB>w2."


class LemmataUnavailableException(EastException):
    """New: the reference declares the 'lemmata' vector space and raises when it is used (relevance.py:98-100)."""
    msg_fmt = "The 'lemmata' vector space has no implementation (nor has the reference's): use '-v words' or '-v stems'."


class StemmerUnavailableException(EastException):
    """New: the 'stems' vector space needs a stemmer; the default is nltk's Snowball stemmer (relevance.py:7, 67-68)."""
    msg_fmt = ("The 'stems' vector space needs nltk's Snowball stemmer, and nltk is not installed: "
               "use '-v words' (or pass a stemmer to CosineRelevanceMeasure).")
