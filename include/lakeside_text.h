/* Host-only test hook: the Java 17 Double.toString / Float.toString text the exemplar path prints for DOUBLE / FLOAT
 * columns (lakeside_amd/csrc/jdtoa.cpp; the reference gets it from DuckDB's JDBC getString, Commons.scala:428-459).
 * Built as lakeside_amd/liblakeside_text.so for the CPU differential tests; the evaluator links the same source.
 * Not part of the drop-in boundary (include/lakeside_gpu.h). */
#ifndef LAKESIDE_TEXT_H
#define LAKESIDE_TEXT_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Writes the NUL-terminated text of x into buf; returns its length, or -1 when cap is too small (32 always fits). */
int lk_java_double_text(double x, char* buf, size_t cap);
int lk_java_float_text(float x, char* buf, size_t cap);

/* The double a field chart aggregates for the text s[0..n) of a VARCHAR chart field (lakeside_amd/csrc/fieldnum.cpp):
 * 1 and *out = the number when the whole text matches -?[0-9]+(\.[0-9]+)?([eE][-+]?[0-9]+)? and is finite; 0 when the
 * cast is NULL (the first byte is an ASCII letter other than i I n N); -1 for every other text, which the evaluator
 * refuses (LK_ERR_UNSUPPORTED) instead of guessing DuckDB's cast.  out may be NULL. */
int lk_field_number(const char* s, size_t n, double* out);

#ifdef __cplusplus
}
#endif
#endif
