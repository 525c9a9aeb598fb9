"""The reference's reading loop, restated as a simulation of an input stream (utils/Bloom.cpp:280-282,340; src/ReadScanner.cpp:306-308,349):

    string read;
    while (getline(in, read)) { getline(in, read); <the read is `read`>; if (fastq) getline(in, read), getline(in, read); }

Imports nothing from the project.  What matters is std::getline's contract, kept here as it stands: a call on a stream that is not good()
(eofbit or failbit set) fails in its sentry and leaves the string ALONE; a call on a good stream erases the string, takes bytes up to the
next '\\n' (which it swallows) or to the end of the text (which sets eofbit), and fails if it took nothing at all.  There is ONE string, so
after a header line that ended with the text the failed call for the sequence leaves the header in it: that header is the record's read.
A read is described by its byte range in the text, whatever it holds.

tests/golden/make_input_golden.py pins this file to the compiled reference with no project code in between."""


class _Stream:
    """an istream over `text`, and the one string of the loop as the byte range [start, end) of the text that it holds"""

    def __init__(self, text):
        self.text = text
        self.pos = 0
        self.eof = self.fail = False
        self.start = self.end = 0           # `read`, empty at first
        self.ended_at_newline = False       # the last successful getline swallowed a '\n'

    def getline(self):
        if self.eof or self.fail:           # the sentry: not good() -> failbit, the string is not touched
            self.fail = True
            return False
        nl = self.text.find(b"\n", self.pos)            # the string is erased, then filled
        self.start = self.pos
        if nl < 0:
            self.end = self.pos = len(self.text)
            self.eof = True
            self.ended_at_newline = False
            if self.end == self.start:                  # nothing extracted
                self.fail = True
        else:
            self.end = nl
            self.pos = nl + 1
            self.ended_at_newline = True
        return not self.fail


def _loop(text, fastq):
    """every iteration of the loop: (start, end) of the read, whether each of its getlines ended at a newline, the position behind it"""
    s = _Stream(bytes(text))
    out = []
    while s.getline():
        whole = s.ended_at_newline
        whole = s.getline() and s.ended_at_newline and whole
        read = (s.start, s.end)
        if fastq:
            whole = s.getline() and s.ended_at_newline and whole
            whole = s.getline() and s.ended_at_newline and whole
        out.append((read, bool(whole), s.pos))
    return out


def records(text, fastq):
    """the byte range (start, end) in `text` of every record's read, `text` being a whole file (or the final chunk of one)"""
    return [r for r, _, _ in _loop(text, fastq)]


def reads(text, fastq):
    text = bytes(text)
    return [text[a:b] for a, b in records(text, fastq)]


def chunk(text, fastq, final):
    """(ranges of the reads handed out, bytes consumed) for one chunk of a file.  A chunk that is not the last one hands out its complete
    records only -- those whose every line ends with a newline inside the chunk -- and the rest is seen again in front of the next chunk"""
    it = _loop(text, fastq)
    if final:
        return [r for r, _, _ in it], len(text)
    done = [(r, pos) for r, whole, pos in it if whole]
    return [r for r, _ in done], (done[-1][1] if done else 0)


def consumed(text, fastq):
    """for a NON-final chunk: the position behind the newline that ends the last complete record, 0 (and no reads) if there is none"""
    return chunk(text, fastq, False)[1]


def cuts(text, lines_per_record, group, n):
    """n + 1 offsets that cut the file into n shards of whole groups of records: cut r is the first position at or behind the nominal
    position size / n * r + size % n * r / n (integer arithmetic) that starts a line whose index is a multiple of lines_per_record * group;
    the size of the file if there is none.  Monotone."""
    text = bytes(text)
    size = len(text)
    period = lines_per_record * max(group, 1)
    line_starts = [0]
    at = text.find(b"\n")
    while at >= 0:
        line_starts.append(at + 1)
        at = text.find(b"\n", at + 1)
    out = [0]
    for r in range(1, n):
        nominal = size // n * r + size % n * r // n
        cut = size
        if size:
            for index in range(0, len(line_starts), period):
                if line_starts[index] >= nominal:
                    cut = line_starts[index]
                    break
        out.append(max(cut, out[-1]))
    out.append(size)
    return out
