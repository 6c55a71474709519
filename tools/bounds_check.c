/* bounds_check.c — a stand-alone host program over oracle/oracle.c: orc_meshlet_bounds on the case arrays of
 * tests/bounds_cases.py (counts beyond the limits, masked index bytes, every reference width, degenerate triangles, fp16 ties,
 * flush and saturation, NaN and infinity in the vertices).  Its own main, no Python in the process; meant for the host sanitizers:
 *   gcc -std=c11 -O1 -g -ffp-contract=off -fopenmp -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all
 *       -static-libasan -static-libubsan -I oracle tools/bounds_check.c oracle/oracle.c -lm -o bounds_check
 *   ./bounds_check cases.bin [results.bin]
 * cases.bin: uint32 {magic 'NVBC', meshlets, data words, vertices}, then the Meshlet records (24 bytes each), the meshlet data
 * words and the Vertex records (16 bytes each) — every array with exactly the size the header states, so that a read past an end
 * is a heap overflow the sanitizer sees.  results.bin (optional): the records after the pass, then eight floats per meshlet.
 * The program also checks what needs no second opinion: bytes 12..23 of every record untouched, the records the same with and
 * without the float output and for any pre-fill of the output fields, and a second pass over its own output changing nothing.
 * Exit status 0 and "bounds_check: ok" when everything holds. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oracle.h"

#define CHECK(c)                                                                \
	do                                                                          \
	{                                                                           \
		if (!(c))                                                               \
		{                                                                       \
			fprintf(stderr, "bounds_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                                           \
		}                                                                       \
	} while (0)

int main(int argc, char** argv)
{
	CHECK(argc >= 2);
	FILE* f = fopen(argv[1], "rb");
	CHECK(f);
	uint32_t header[4];
	CHECK(fread(header, 4, 4, f) == 4 && header[0] == 0x4342564eu);
	const uint32_t count = header[1], words = header[2], nvert = header[3];
	CHECK(sizeof(OrcMeshlet) == 24 && sizeof(OrcVertex) == 16);
	OrcMeshlet* input = malloc((size_t)count * sizeof(OrcMeshlet));
	uint32_t* data = malloc((size_t)words * 4);
	OrcVertex* vertices = malloc((size_t)nvert * sizeof(OrcVertex));
	CHECK(input && data && vertices);
	CHECK(fread(input, sizeof(OrcMeshlet), count, f) == count && fread(data, 4, words, f) == words && fread(vertices, sizeof(OrcVertex), nvert, f) == nvert);
	CHECK(fgetc(f) == EOF);
	fclose(f);

	OrcMeshlet* a = malloc((size_t)count * sizeof(OrcMeshlet));
	OrcMeshlet* b = malloc((size_t)count * sizeof(OrcMeshlet));
	float* out8 = malloc((size_t)count * 8 * sizeof(float));
	CHECK(a && b && out8);
	memcpy(a, input, (size_t)count * sizeof(OrcMeshlet));
	orc_meshlet_bounds(vertices, data, a, count, out8);
	/* without the float output, the output fields zeroed first */
	memcpy(b, input, (size_t)count * sizeof(OrcMeshlet));
	for (uint32_t i = 0; i < count; ++i)
		memset(&b[i], 0, 12);
	orc_meshlet_bounds(vertices, data, b, count, NULL);
	CHECK(memcmp(a, b, (size_t)count * sizeof(OrcMeshlet)) == 0);
	for (uint32_t i = 0; i < count; ++i)
		CHECK(memcmp((const char*)&a[i] + 12, (const char*)&input[i] + 12, 12) == 0);
	/* a second pass over its own output */
	orc_meshlet_bounds(vertices, data, b, count, NULL);
	CHECK(memcmp(a, b, (size_t)count * sizeof(OrcMeshlet)) == 0);
	/* one meshlet at a time, from exact-size copies of a single record */
	for (uint32_t i = 0; i < count; i += 7)
	{
		OrcMeshlet* one = malloc(sizeof(OrcMeshlet));
		float* o8 = malloc(8 * sizeof(float));
		CHECK(one && o8);
		*one = input[i];
		orc_meshlet_bounds(vertices, data, one, 1, o8);
		CHECK(memcmp(one, &a[i], sizeof(OrcMeshlet)) == 0 && memcmp(o8, out8 + (size_t)i * 8, 32) == 0);
		free(one);
		free(o8);
	}
	if (argc >= 3)
	{
		FILE* o = fopen(argv[2], "wb");
		CHECK(o);
		CHECK(fwrite(a, sizeof(OrcMeshlet), count, o) == count && fwrite(out8, 32, count, o) == count);
		CHECK(fclose(o) == 0);
	}
	free(input), free(data), free(vertices), free(a), free(b), free(out8);
	printf("bounds_check: ok (%u meshlets)\n", count);
	return 0;
}
