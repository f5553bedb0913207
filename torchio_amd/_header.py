"""Reader of ``include/tio_hip.h``: the constants, struct layouts and prototypes of the C ABI as ``ctypes`` sees them.

The header is the one description of the ABI; ``_abi`` derives its tables from what this module reads, so the two cannot
drift apart.  The reader knows exactly the C the header is written in and **fails closed**: anything else raises
``HeaderError`` quoting the declaration, instead of being skipped.

Grammar, after ``/* */`` and ``//`` comments are removed:

* directives: ``#include <x.h>``; ``#ifndef NAME`` of a name not yet defined (the include guard) and its ``#endif``;
  ``#ifdef __cplusplus`` ... ``#endif``, dropped as a C compiler drops it; ``#define NAME`` (no value: no constant);
  ``#define NAME(...) ...`` (function-like: text substitution, no constant); ``#define NAME literal`` with an integer or
  floating literal, a constant;
* ``typedef enum tag { NAME = integer, ... } tag;`` — every member a constant;
* ``typedef struct tag { fields } tag;`` with fields ``T name;``, ``T name[N];``, ``T* name;`` and ``T a, b;``, ``T`` a
  fixed-width scalar (``SCALARS``; ``void`` behind a pointer) and ``N`` an integer, a constant or ``CONSTANT / integer``;
  no bit-fields, no nested structs;
* ``ret tio_name(parameters);`` with ``ret`` one of ``RETURNS``, parameters ``T name``, ``T name[N]``, ``T* name``
  (``const`` anywhere a pointer allows it) or the single word ``void``, ``T`` a scalar, ``void`` or a struct declared above.

How a parameter maps to ``ctypes`` (``Header.prototypes``):

* a scalar maps to its exact type in ``SCALARS``;
* an array parameter ``T x[N]`` maps to ``POINTER(T)``;
* a pointer to a struct of which the caller hands in a class maps to ``POINTER(thatClass)``;
* every other pointer maps to ``c_void_p``.

Struct fields map alike, except that every pointer field is a ``c_void_p`` and an array field is ``T * N``.
"""
from __future__ import annotations

import ctypes as C
import keyword
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tio_hip.h")

SCALARS = {
    "int": C.c_int,
    "int8_t": C.c_int8, "uint8_t": C.c_uint8,
    "int32_t": C.c_int32, "uint32_t": C.c_uint32,
    "int64_t": C.c_int64, "uint64_t": C.c_uint64,
    "float": C.c_float, "double": C.c_double,
}  # fmt: skip
RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p, "void": None}

_INTEGER = re.compile(r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+)")
_FLOATING = re.compile(r"[-+]?(?:\d+\.\d*(?:[eE][-+]?\d+)?|\d+[eE][-+]?\d+)")
_TYPEDEF = re.compile(r"typedef\s+(enum|struct)\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTOTYPE = re.compile(r"([\w\s*]+?)\s*\b(\w+)\s*\(([^()]*)\)\s*;")
_SPACE = re.compile(r"\s*")
_TYPE = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)")  # the type word and its stars
_DECLARATOR = re.compile(r"(\w+)\s*(?:\[([^\[\]]+)\])?")  # name, array length


class HeaderError(ValueError):
    """The header holds a declaration outside the grammar this module reads."""


class Header:
    """What the header's text declares, names as the header spells them.

    ``constants``: name -> int | float.  ``structs``: tag -> [(type, stars, name, length | None)], ``stars`` the depth of
    the pointer (0: a value).  ``functions``: name without ``tio_`` -> (return type, [one such tuple per parameter])."""

    def __init__(self, text: str, path: str = HEADER_PATH):
        self.path = path
        self.constants: dict = {}
        self.structs: dict = {}
        self.functions: dict = {}
        self._valueless: set = set()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        self._declarations(self._directives(text.split("\n")))

    def _error(self, why: str, declaration: str):
        return HeaderError(f"{self.path}: {why}: {declaration.strip()}")

    def _constant(self, name: str, value, declaration: str) -> None:
        """``value`` None: a ``#define`` without one, which makes no constant."""
        if name in self.constants or name in self._valueless:
            raise self._error(f"{name} is defined twice", declaration)
        if value is None:
            self._valueless.add(name)
        else:
            self.constants[name] = value

    def _directives(self, lines) -> str:
        """Take the ``#`` lines; return the text a C compiler is left with."""
        body, guards, in_cplusplus = [], 0, False
        for line in lines:
            directive = re.fullmatch(r"#\s*(\w+)\s*(.*)", line.strip())
            if directive is None:
                if line.lstrip().startswith("#"):
                    raise self._error("directive not understood", line)
                if not in_cplusplus:
                    body.append(line)
                continue
            word, rest = directive.groups()
            if word == "endif" and not rest and in_cplusplus:
                in_cplusplus = False
            elif word == "endif" and not rest and guards:
                guards -= 1
            elif in_cplusplus:
                raise self._error("directive inside #ifdef __cplusplus", line)
            elif word == "ifdef" and rest == "__cplusplus":
                in_cplusplus = True
            elif word == "ifndef" and re.fullmatch(r"\w+", rest) and rest not in self.constants and rest not in self._valueless:
                guards += 1
            elif word == "include" and re.fullmatch(r"<\w+\.h>", rest):
                pass
            elif word == "define" and (define := re.fullmatch(r"(\w+)(\()?\s*(.*)", rest)):
                name, function_like, value = define.groups()
                if function_like:
                    continue
                if not value:
                    self._constant(name, None, line)
                elif _INTEGER.fullmatch(value):
                    self._constant(name, int(value, 0), line)
                elif _FLOATING.fullmatch(value):
                    self._constant(name, float(value), line)
                else:
                    raise self._error("the value of a #define must be an integer or floating literal", line)
            else:
                raise self._error("directive not understood", line)
        if guards or in_cplusplus:
            raise self._error("unterminated conditional", "#endif")
        return "\n".join(body)

    def _declarations(self, text: str) -> None:
        position = 0
        while (position := _SPACE.match(text, position).end()) < len(text):
            if typedef := _TYPEDEF.match(text, position):
                kind, tag, body, name = typedef.groups()
                if tag != name or name in self.structs:
                    raise self._error("a typedef names its own tag, once", typedef.group(0))
                if kind == "enum":
                    for member in body.split(","):
                        if not (parts := re.fullmatch(r"\s*(\w+)\s*=\s*(\S+)\s*", member)) or not _INTEGER.fullmatch(parts.group(2)):
                            raise self._error("an enum member is NAME = integer", typedef.group(0))
                        self._constant(parts.group(1), int(parts.group(2), 0), typedef.group(0))
                else:
                    *fields, rest = body.split(";")
                    if rest.strip():
                        raise self._error("field without a semicolon", rest)
                    self.structs[tag] = [entry for field in fields for entry in self._declare(field, field + ";", many=True)]
                position = typedef.end()
            elif prototype := _PROTOTYPE.match(text, position):
                whole = prototype.group(0)
                returns, name, parameters = prototype.groups()
                returns = re.sub(r"\s*\*", "*", " ".join(returns.split()))
                if returns not in RETURNS:
                    raise self._error(f"return type {returns!r} is none of {sorted(RETURNS)}", whole)
                if not name.startswith("tio_") or name[4:] in self.functions:
                    raise self._error("an entry point is named tio_*, once", whole)
                if not parameters.strip():
                    raise self._error("an empty parameter list is spelled (void)", whole)
                parameters = [] if parameters.strip() == "void" else parameters.split(",")
                self.functions[name[4:]] = (returns, [self._declare(parameter, whole)[0] for parameter in parameters])
                position = prototype.end()
            else:
                end = text.find("\n", max(text.find(";", position), position))  # through the line of the next semicolon
                raise self._error("declaration not understood", text[position : end if end >= 0 else len(text)])

    def _declare(self, text: str, quoted: str, many: bool = False) -> list:
        """``T name``, ``T* name``, ``T name[N]`` (``many``: ``T a, b``) -> [(type, stars, name, length | None)]."""
        text = text.strip()
        head = _TYPE.match(text)
        if head is None:
            raise self._error("declaration not understood", quoted)
        type_name, pointer = head.group(1), head.group(2).count("*")
        if type_name not in SCALARS and not (type_name == "void" and pointer) and type_name not in self.structs:
            raise self._error(f"unknown type {type_name!r}", quoted)
        declared = []
        for item in text[head.end() :].split(","):
            declarator = _DECLARATOR.fullmatch(item.strip())
            if declarator is None or (declared and not many):
                raise self._error("declaration not understood", quoted)
            name, length = declarator.groups()
            if length is not None:
                if pointer:
                    raise self._error("array of pointers", quoted)
                length = self._length(length.strip(), quoted)
            if type_name in self.structs and not pointer and (many or length is None):
                raise self._error("nested struct" if many else "struct passed by value", quoted)
            declared.append((type_name, pointer, name, length))
        return declared

    def _length(self, text: str, quoted: str) -> int:
        parts = re.fullmatch(r"(\w+)(?:\s*/\s*(\d+))?", text)
        if parts and parts.group(1).isdigit():
            value = int(parts.group(1))
        elif parts and isinstance(self.constants.get(parts.group(1)), int):
            value = self.constants[parts.group(1)]
        else:
            raise self._error("an array length is an integer, a constant or CONSTANT / integer", quoted)
        return value // int(parts.group(2) or 1)

    def struct_class(self, tag: str, class_name: str) -> type:
        """A ``ctypes.Structure`` laid out like ``tag``; a field named like a Python keyword gets a trailing underscore."""
        fields = []
        for type_name, pointer, name, length in self.structs[tag]:
            ctype = C.c_void_p if pointer else SCALARS[type_name]
            fields.append((name + "_" * keyword.iskeyword(name), ctype if length is None else ctype * length))
        return type(class_name, (C.Structure,), {"_fields_": fields, "__doc__": f"``{tag}``."})

    def prototypes(self, classes: dict) -> dict:
        """name -> (restype, argtypes) for every entry point, by the module's parameter rule; ``classes``: tag -> class."""
        table = {}
        for name, (returns, parameters) in self.functions.items():
            argtypes = []
            for type_name, pointer, parameter, length in parameters:
                element = classes.get(type_name) or SCALARS.get(type_name)
                if length is not None or (pointer == 1 and type_name in classes):
                    if element is None:
                        raise self._error(f"array parameter of a struct without a class, {type_name}", f"tio_{name}: {parameter}")
                    argtypes.append(C.POINTER(element))
                else:
                    argtypes.append(C.c_void_p if pointer else SCALARS[type_name])
            table[name] = (RETURNS[returns], argtypes)
        return table


def load(path: str = HEADER_PATH) -> Header:
    try:
        with open(path, encoding="utf-8") as file:
            text = file.read()
    except OSError as error:
        raise ImportError(f"cannot read the C ABI header {path}: {error}") from error
    return Header(text, path)
