// TEST INFRASTRUCTURE ONLY: the parameter-file reader behind the reference program's interface (see ParseHeader.hh).
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "ParseHeader.hh"

namespace {

struct ParseError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

[[noreturn]] void fail(const std::string &what) { throw ParseError(what); }

// split the right-hand side of a definition into tokens; `quoted` records which came in quotes
void tokens_of(const std::string &rhs, int lineno, std::vector<std::string> &tok, std::vector<bool> &quoted) {
    size_t i = 0;
    while (i < rhs.size()) {
        if (isspace((unsigned char) rhs[i])) {
            i++;
        } else if (rhs[i] == '"') {
            size_t e = rhs.find('"', i + 1);
            if (e == std::string::npos) fail(fmt::format("line {}: unterminated string", lineno));
            tok.push_back(rhs.substr(i + 1, e - i - 1));
            quoted.push_back(true);
            i = e + 1;
        } else {
            size_t e = i;
            while (e < rhs.size() && !isspace((unsigned char) rhs[e]) && rhs[e] != '"') e++;
            tok.push_back(rhs.substr(i, e - i));
            quoted.push_back(false);
            i = e;
        }
    }
}

long long integer_of(const std::string &key, const std::string &t) {
    errno = 0;
    char *end;
    long long v = strtoll(t.c_str(), &end, 10);
    if (t.empty() || *end || errno) fail(fmt::format("{}: \"{}\" is not an integer", key, t));
    return v;
}

double double_of(const std::string &key, std::string t) {
    for (char &c : t)  // Fortran exponents
        if (c == 'd' || c == 'D') c = 'e';
    errno = 0;
    char *end;
    double v = strtod(t.c_str(), &end);
    if (t.empty() || *end || errno == ERANGE) fail(fmt::format("{}: \"{}\" is not a number", key, t));
    return v;
}

}  // namespace

HeaderStream::HeaderStream(const fs::path &fn) : name(fn), fp(NULL) {
    fp = fopen(fn.c_str(), "rb");
    if (fp == NULL) {
        fmt::print(stderr, "HeaderStream: cannot open \"{}\": {}\n", fn.string(), strerror(errno));
        exit(1);
    }
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, n);
}

HeaderStream::~HeaderStream(void) { Close(); }

void HeaderStream::Close(void) {
    if (fp != NULL) fclose(fp);
    fp = NULL;
}

void WriteHStream(FILE *fp, const std::string &m, const std::string &pre) {
    size_t i = 0;
    while (i < m.size()) {
        size_t e = m.find('\n', i);
        if (e == std::string::npos) e = m.size();
        fmt::print(fp, "{}{}\n", pre, m.substr(i, e - i));
        i = e + 1;
    }
}
void WriteHStream(FILE *fp, const std::string &m) { WriteHStream(fp, m, ""); }
void WriteHStream(FILE *fp, HeaderStream &in, const std::string &pre) { WriteHStream(fp, in.text, pre); }
void WriteHStream(FILE *fp, HeaderStream &in) { WriteHStream(fp, in.text, ""); }

void ParseHeader::install(const std::string &name, Kind kind, void *var, bool is_vector, bool must_define, size_t maxlen) {
    if (syms.count(name)) {
        fmt::print(stderr, "ParseHeader: \"{}\" registered twice\n", name);
        exit(1);
    }
    if (is_vector && kind != K_INT) {
        fmt::print(stderr, "ParseHeader: vector \"{}\": only vectors of int are supported\n", name);
        exit(1);
    }
    syms[name] = Sym{kind, var, is_vector, must_define, false, maxlen};
}

void ParseHeader::ReadHeader(HeaderStream &in) {
    std::string err = ParseText(in.text);
    if (!err.empty()) {
        fmt::print(stderr, "ParseHeader: {}: {}\n", in.name.string(), err);
        exit(1);
    }
}

std::string ParseHeader::ParseText(const std::string &text) {
    try {
        size_t pos = 0;
        int lineno = 0;
        while (pos < text.size()) {
            size_t e = text.find('\n', pos);
            if (e == std::string::npos) e = text.size();
            std::string line = text.substr(pos, e - pos);
            pos = e + 1;
            lineno++;
            bool inq = false;  // a '#' inside quotes is text
            for (size_t i = 0; i < line.size(); i++) {
                if (line[i] == '"') inq = !inq;
                if (line[i] == '#' && !inq) {
                    line.resize(i);
                    break;
                }
            }
            size_t b = line.find_first_not_of(" \t\r");
            if (b == std::string::npos) continue;
            size_t eq = line.find('=');
            if (eq == std::string::npos) fail(fmt::format("line {}: no '=' in \"{}\"", lineno, line));
            std::string key = line.substr(b, eq - b);
            key.erase(key.find_last_not_of(" \t") + 1);
            if (key.empty() || key.find_first_of(" \t\"") != std::string::npos)
                fail(fmt::format("line {}: bad key \"{}\"", lineno, key));
            auto it = syms.find(key);
            if (it == syms.end()) fail(fmt::format("line {}: \"{}\" is not a registered parameter", lineno, key));
            Sym &s = it->second;
            if (s.seen) fail(fmt::format("line {}: \"{}\" defined twice", lineno, key));
            s.seen = true;
            std::vector<std::string> tok;
            std::vector<bool> quoted;
            tokens_of(line.substr(eq + 1), lineno, tok, quoted);
            if (tok.empty()) fail(fmt::format("line {}: \"{}\" has no value", lineno, key));
            if (s.is_vector) {
                std::vector<int> &v = *(std::vector<int> *) s.var;
                if (tok.size() > s.maxlen) fail(fmt::format("{}: more than {} values", key, s.maxlen));
                v.clear();
                for (size_t i = 0; i < tok.size(); i++) {
                    if (quoted[i]) fail(fmt::format("{}: a string in a vector of integers", key));
                    v.push_back((int) integer_of(key, tok[i]));
                }
                continue;
            }
            if (tok.size() != 1) fail(fmt::format("line {}: \"{}\" takes one value, {} given", lineno, key, tok.size()));
            bool text_kind = s.kind == K_STRING || s.kind == K_PATH;
            if (text_kind != (bool) quoted[0])
                fail(fmt::format("line {}: \"{}\" {} a quoted string", lineno, key, text_kind ? "needs" : "cannot take"));
            switch (s.kind) {
                case K_DOUBLE: *(double *) s.var = double_of(key, tok[0]); break;
                case K_INT: {
                    long long v = integer_of(key, tok[0]);
                    if (v != (int) v) fail(fmt::format("{}: {} does not fit an int", key, v));
                    *(int *) s.var = (int) v;
                    break;
                }
                case K_LONGLONG: *(long long *) s.var = integer_of(key, tok[0]); break;
                case K_STRING: *(std::string *) s.var = tok[0]; break;
                case K_PATH: *(fs::path *) s.var = fs::path(tok[0]); break;
            }
        }
        for (auto &kv : syms)
            if (kv.second.must_define && !kv.second.seen) fail(fmt::format("\"{}\" must be defined", kv.first));
    } catch (const ParseError &e) {
        return e.what();
    }
    return "";
}
