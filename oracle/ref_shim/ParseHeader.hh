// TEST INFRASTRUCTURE ONLY.  This project's stand-in for the parameter-file reader the reference program is written
// against: the two classes and the calls its sources make, nothing of the original's flex / bison grammar.  Grammar:
// one `key = value ...` per line, `#` comments, "quoted strings", whitespace-separated vectors, Fortran exponents
// (1.5d3) for doubles.  A key that must be defined and is missing, a key nobody registered, a second definition and
// a value of the wrong type all end the program with status 1.
#ifndef ZD_SHIM_PARSEHEADER_HH
#define ZD_SHIM_PARSEHEADER_HH

#include <cstdio>
#include <filesystem>
#include <map>
#include <string>
#include <vector>

#include <fmt/format.h>
#include <fmt/std.h>

namespace fs = std::filesystem;

#define MUST_DEFINE true
#define DONT_CARE false

class HeaderStream {
public:
    HeaderStream(const fs::path &fn);
    virtual ~HeaderStream(void);
    void Close(void);

    fs::path name;
    FILE *fp;
    std::string text;  // the whole header as read
};

void WriteHStream(FILE *fp, const std::string &m);
void WriteHStream(FILE *fp, const std::string &m, const std::string &pre);
void WriteHStream(FILE *fp, HeaderStream &in);
void WriteHStream(FILE *fp, HeaderStream &in, const std::string &pre);

class ParseHeader {
public:
    enum Kind { K_DOUBLE, K_INT, K_LONGLONG, K_STRING, K_PATH };

    template <typename T>
    void installscalar(const std::string &name, T &var, bool must_define) {
        install(name, kind_of(&var), &var, false, must_define, 1);
    }
    template <typename T>
    void installvector(const std::string &name, std::vector<T> &var, bool must_define, size_t maxlen = 1024) {
        install(name, kind_of((T *) 0), &var, true, must_define, maxlen);
    }
    void ReadHeader(HeaderStream &in);                // ends the program with status 1 on any error
    std::string ParseText(const std::string &text);  // the same without the exit: "" or what is wrong

private:
    struct Sym {
        Kind kind;
        void *var;
        bool is_vector, must_define, seen;
        size_t maxlen;
    };
    std::map<std::string, Sym> syms;

    static Kind kind_of(double *) { return K_DOUBLE; }
    static Kind kind_of(int *) { return K_INT; }
    static Kind kind_of(long long *) { return K_LONGLONG; }
    static Kind kind_of(std::string *) { return K_STRING; }
    static Kind kind_of(fs::path *) { return K_PATH; }
    void install(const std::string &name, Kind kind, void *var, bool is_vector, bool must_define, size_t maxlen);
};

#endif
